/* qtcnn.h -- C ABI of the MI355X (gfx950) QuadtreeCNN hot-path library.
 *
 * The reference (Avirup221/Multimodal-Hierarchical-CNN-for-Sun-Salutation-Pose-
 * Classification) has no FFI of its own: its hot path is torch.nn modules calling
 * ATen.  This header is the boundary a maintainer binds instead (ctypes stub in
 * INTEGRATION.md).  Every entry point names the reference call it replaces.
 *
 * Conventions
 *   - plain C types only; every pointer is a DEVICE pointer unless it says "host";
 *   - the caller owns every buffer (including workspaces); the library allocates
 *     nothing persistent on the device.  Process-wide state is limited to (i) the
 *     kernel-selection switches qt_set_patch_conv / qt_set_pt_conv / qt_set_stem_conv /
 *     qt_set_wgrad_patch_min_width / qt_set_wgrad_patch_variant and the QTCNN_* environment variables they mirror
 *     (read once; DESIGN.md section 5 lists them) -- they pick between kernels that
 *     compute the same result, set them before the first launch -- and (ii) the
 *     per-device "LDS limit raised" bits of the large-LDS kernels;
 *   - the per-op entry points enqueue all work on `stream` (a hipStream_t passed as
 *     void*) with no internal synchronisation and are re-entrant across streams.  A
 *     qt_plan additionally OWNS one side stream and a handful of events (created in
 *     qt_plan_create, destroyed in qt_plan_destroy): qt_plan_backward forks the
 *     weight-gradient launches onto it and joins them back into `stream` before it
 *     returns (qt_plan_side_fence exposes the join to another stream).  One plan is
 *     used by one host thread at a time; one process per GPU under data parallelism;
 *   - return value: QT_OK (0) or a negative qt_status; qt_last_error() returns a
 *     thread-local description of the last failure; nothing throws across the ABI;
 *   - activations are NHWC, element type qt_dtype (bf16 throughput build or the
 *     f32 parity build of the SAME kernels); accumulation is always f32 on MFMA.
 */
#ifndef QTCNN_H_
#define QTCNN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum qt_status {
  QT_OK = 0,
  QT_ERR_INVALID_ARG = -1,
  QT_ERR_LAUNCH = -2,
  QT_ERR_UNSUPPORTED = -3
} qt_status;

typedef enum qt_dtype { QT_F32 = 0, QT_BF16 = 1 } qt_dtype;

int qt_version(void);
const char* qt_last_error(void);

/* ------------------------------------------------------------------------
 * Implicit-GEMM convolution on MFMA.
 *   QT_CONV_FWD   replaces nn.Conv2d forward   (ResNet-18 convs reached at
 *                 Quadtree_from scratch/models.py:222-230,241; the quadrant conv
 *                 :235 called 4x at :284-287; resnet/models.py:80-100,158-161)
 *   QT_CONV_DGRAD replaces the conv backward-input ATen call that loss.backward()
 *                 (Quadtree_from scratch/Quadtree_train.py:65) makes per conv.
 * dst[m][n] = epilogue( sum_{tap,k} W[n][tap][k] * src[pixel(m) moved by tap][k] )
 * epilogue(v) = relu_mask( relu( v*scale[n] + shift[n] + residual[m][n] ) ),
 * each part optional; stats_partial (optional) receives per-128-row-tile sums and
 * sums of squares of the raw v per channel: [qt_conv2d_stats_rows][2][n_out] f32.
 * Non-finite values (every forward entry point of this header, not only this one): dst
 * holds NaN, +inf and -inf where IEEE arithmetic on the same operands gives them, in any
 * order of summation; relu is the NaN-propagating maximum (relu(NaN) = NaN as torch.relu,
 * relu(-0.0) = +0.0), never fmaxf.  The max pools (qt_stem_pool, qt_stem_conv_pool*,
 * qt_quad_pool, qt_pool3d_max, qt_pool3d_bn_relu_max, qt_conv3d_first_fwd_pool) follow
 * ATen: a NaN wins every comparison, so a window that holds one pools to NaN and its
 * argmax is the LAST NaN in scan order.  The backward ReLU gates (relu_mask,
 * relu_mask_bits as qt_bn_act_mask writes them, the gates the fused backward kernels
 * recompute) are torch's threshold_backward: the gradient is dropped where act <= 0
 * (+0.0 and -0.0 alike) and kept otherwise, at a NaN activation too.
 * ------------------------------------------------------------------------ */
enum { QT_CONV_FWD = 0, QT_CONV_DGRAD = 1 };

typedef struct qt_conv_desc {
  int dtype;         /* qt_dtype of src / weight / dst / residual / relu_mask */
  int mode;          /* QT_CONV_FWD or QT_CONV_DGRAD */
  int batch;         /* images */
  int in_h, in_w;    /* spatial size of src (per quadrant when quad != 0) */
  int out_h, out_w;  /* spatial size of dst (per quadrant for quad FWD) */
  int k_per_tap;     /* contracted channels per tap; multiple of 64 (bf16) / 32 (f32) */
  int n_out;         /* channels of dst; multiple of 8 */
  int kh, kw, stride, pad;
  long long src_img_stride; /* elements between images of src */
  int src_row_stride;       /* elements between rows of src */
  int src_pix_stride;       /* elements between pixels of src */
  int quad;  /* S = 2 (1 means 2) or 4: FWD reads the S x S regions of a (S*in_h x S*in_w) map as
                S*S*batch images (region rr*S+rc of image n is image n*S*S + rr*S + rc) with zero halo
                at the seams (Quadtree_from scratch/models.py:277-287 quadrants; :62-78 quadrants and
                sub-quadrants of AttentionHierarchicalCNN); DGRAD scatters the per-region gradient
                images back onto the un-split map */
  int relu;
  /* optional strided destination (0 = dense [M][n_out]): row (img, oh, ow) is written to pixel
   * (oh*dst_sub + dst_off_h, ow*dst_sub + dst_off_w) of a dst_h x dst_w image; residual and
   * relu_mask are read at the same place.  Used to run the data gradient of a stride-2 conv as
   * four stride-1 gathers, one per output-pixel parity class (qt_pack_dgrad_s2). */
  int dst_sub, dst_h, dst_w, dst_off_h, dst_off_w;
  /* dst_merge = C > 0 (with dst_sub = 2, n_out = 4*C): the n_out channels of a row are the FOUR parity classes of a
   * stride-2 data gradient at once -- channel n is channel n % C of pixel (2*oh + (n/C >> 1), 2*ow + (n/C & 1)) of the
   * dst_h x dst_w image with C channels; residual / relu_mask / BatchNorm links are read there and the link sums
   * are written as 4 partial rows of C channels per pixel tile.  One 2x2-tap launch over the gradient map instead of
   * four gathers that each re-read it (weight operand: qt_pack_dgrad_s2_merged). */
  int dst_merge;
  int dst_merge_res0;  /* with dst_merge: the residual is added to class (0,0) only (the other pixels of it are never read) */
  /* Conv3d as ONE launch (nn.Conv3d 3x3x3 / pad 1 of /root/reference/3dcnn/models.py:108-139, cnn+lstm/models.py:104-121):
   * kt = 3 frame taps on time-major clips [frames][batch / frames][H][W][C] -- `batch` counts images = frames x clips,
   * image t * (batch / frames) + b is frame t of clip b; tap (kt, kh, kw) of an output image reads the image one frame
   * earlier / same / later (zero where that frame does not exist), weight [n_out][kt][kh][kw][k_per_tap]; f32
   * accumulation over all kt * kh * kw taps, the epilogue (bias, residual, BatchNorm3d statistics) sees the finished value.
   * DGRAD mirrors it.  Needs stride 1 and no region / strided-destination mode; 0 or 1 = plain 2-D. */
  int kt, frames;
  /* With dst_merge: 1 = a FIFTH tap slot (weight rows then hold 5 slots of k_per_tap) that reads qt_conv_io.extra_src -- a
   * second gradient map of the same geometry as src -- at the window's first pixel (r, c) and only reaches class (0,0): the
   * data gradient of the block's 1x1 / stride-2 downsample (torchvision BasicBlock.downsample) accumulated in
   * the same launch as conv1's, instead of a launch of its own whose output the merged launch then re-reads as a residual. */
  int dst_merge_extra;
} qt_conv_desc;

typedef struct qt_conv_io {
  const void* src;
  const void* weight;    /* [n_out][kh*kw][k_per_tap], K contiguous */
  void* dst;             /* [M][n_out] */
  const float* scale;    /* [n_out] or NULL */
  const float* shift;    /* [n_out] or NULL */
  const void* residual;  /* [M][n_out] or NULL */
  const void* relu_mask; /* [M][n_out] or NULL: dst = mask > 0 ? dst : 0 */
  float* stats_partial;  /* or NULL */
  /* Optional (data-gradient launches): up to two BatchNorms consume the value g written to
   * dst; the epilogue then also emits, per 128-row tile, sum g and sum g*(y-mean)*invstd for
   * each of them ([qt_conv2d_stats_rows][2][n_out] f32), which is what qt_bn_bwd_finalize
   * takes -- the separate qt_bn_bwd_reduce pass over g and y is not needed. */
  struct {
    const void* y;       /* BatchNorm input saved by the forward pass, [M][n_out] */
    const float* mean;   /* [n_out] */
    const float* invstd; /* [n_out] */
    float* partial;
  } bwd_bn[2];
  /* The ReLU mask as ONE BIT per element instead of a tensor of the data type: [M][n_out / 8] bytes, bit (n & 7) of byte
   * n / 8 of row m set = the gradient passes (what qt_bn_act_mask writes next to the activation).  NULL or exclusive with
   * relu_mask; read at the destination row like relu_mask (strided / merged destinations included).  n_out % 8 == 0.
   * 1/16 of the bytes of a bf16 mask: the mask is the second-largest epilogue operand of a data-gradient launch. */
  const unsigned char* relu_mask_bits;
  const void* extra_src;  /* qt_conv_desc.dst_merge_extra: [batch][in_h][in_w][k_per_tap] with src's strides, or NULL */
} qt_conv_io;

/* The 56x56 64->64 bf16 3x3 stride-1 convs (ResNet layer1) on the persistent sliding-ring kernel with the input window
 * resident in LDS (csrc/conv_patch.hip) instead of the generic implicit GEMM: 0 never, anything else (default) on.
 * (Rounds 1-3 had an experimental one-tile-per-workgroup kernel behind mode 1; removed in round 4.) */
void qt_set_patch_conv(int mode);
/* 3x3 / stride 1 / pad 1 convolutions on dense 28x28, 14x14 and 7x7 maps with >= 16 images and a multiple of 128 output
 * channels (the twelve such convs of layer2..4, forward and data gradient) take the patch-resident ping-pong kernel
 * (csrc/conv_pt.hip: 196-pixel tiles of whole image rows, input patch + halo of a 128-byte channel chunk in LDS for all
 * nine taps, weight tiles streamed through an LDS-DMA ring, two wave groups half a period apart).  1 (default) on,
 * 0 generic implicit GEMM.  Same arithmetic (f32 accumulation on MFMA) in a different K order: chunk-major, tap-minor;
 * qt_conv2d_stats_rows follows the choice (two rows per 196-pixel tile: one per wave row). */
void qt_set_pt_conv(int mode);
/* The 128-channel-tile instantiations of that kernel are PERSISTENT: one workgroup per CU walks consecutive (channel tile,
 * pixel tile) items without stopping the K-tile stream (the 28x28 stage of the benchmark: four items per workgroup).
 * tests: cap the grid at n workgroups (0 = one per CU; a huge n = one item per workgroup, QTCNN_PT_PERSIST=0 does the
 * same): results are bit-identical for every n. */
void qt_set_pt_conv_max_workgroups(int n);
/* The packed bf16 stem convolution (desc of qt_pack_stem_input: kh 7|8, kw 1, stride 2, k_per_tap 32,
 * 64 outputs, no residual / mask / bwd_bn) takes a dedicated kernel (csrc/conv_stem.hip: input
 * rows of a 4 x 112 pixel tile in LDS, filter in registers, one partial-statistics row per
 * workgroup).  1 (default) on, 0 generic implicit GEMM. */
void qt_set_stem_conv(int mode);
int qt_conv2d_stats_rows(const qt_conv_desc* desc);
/* ---------------------------------------------------------------------------
 * The stride-2 transition of a ResNet stage in ONE launch (csrc/conv_s2.hip): conv1 of layerN.0 (3x3 / stride 2 / pad 1,
 * no bias) and its downsample (1x1 / stride 2, no bias) computed from one staged input patch -- torchvision BasicBlock
 * with `downsample`, i.e. the nn.Conv2d calls behind /root/reference/Quadtree_from scratch/models.py:
 * 228-229,241 (layer2.0, layer3.0, layer4.0) and resnet/models.py:86-88,99.  Replaces two qt_conv2d_igemm launches.
 *   y_conv = epi_conv(conv3x3s2(x, w_conv)),  y_down = epi_down(conv1x1s2(x, w_down)),
 *   epi(v) = relu?(v * scale[c] + shift[c]) with every part optional; stats_* (optional) receive per (pixel tile, wave row)
 *   sums and sums of squares of the RAW v per channel: [qt_conv_s2_pair_stats_rows][2][c_out] f32 (qt_bn_finalize's input).
 * x: NHWC [batch][in_h][in_w][c_in]; w_conv: [c_out][3][3][c_in] (qt_pack_conv_weight's forward operand); w_down:
 * [c_out][c_in]; y_*: NHWC [batch][in_h/2][in_w/2][c_out].  Supported (qt_conv_s2_pair_supported): in_h == in_w in
 * {56, 28, 14}, c_in a multiple of 64 (bf16) / 32 (f32), c_out a multiple of 128, batch >= 16 (a multiple of 4 for
 * 14x14 inputs); other problems take qt_conv2d_igemm.  Same arithmetic as the generic path (f32 accumulation on MFMA)
 * in another K order.  QTCNN_S2_CONV=0 / qt_set_conv_s2(0): report "unsupported" (same-box A/B against the generic pair).
 * ------------------------------------------------------------------------ */
typedef struct qt_conv_s2_desc {
  int dtype;            /* qt_dtype of x, the weights and both outputs */
  int batch;
  int in_h, in_w;
  int c_in, c_out;
  int relu_conv, relu_down;
} qt_conv_s2_desc;
typedef struct qt_conv_s2_io {
  const void* src;
  const void* w_conv;
  const void* w_down;
  void* y_conv;
  void* y_down;
  const float* scale_conv;  /* [c_out] or NULL */
  const float* shift_conv;
  const float* scale_down;
  const float* shift_down;
  float* stats_conv;        /* or NULL */
  float* stats_down;
} qt_conv_s2_io;
int qt_conv_s2_pair_supported(const qt_conv_s2_desc* desc);
int qt_conv_s2_pair_stats_rows(const qt_conv_s2_desc* desc);
int qt_conv_s2_pair(const qt_conv_s2_desc* desc, const qt_conv_s2_io* io, void* stream);
void qt_set_conv_s2(int mode);
/* tests: cap the persistent grid (0 = one workgroup per CU) so that small batches exercise several items per workgroup */
void qt_set_conv_s2_max_workgroups(int n);

int qt_conv2d_igemm(const qt_conv_desc* desc, const qt_conv_io* io, void* stream);

/* Weight gradient of the convolution described by `desc` (mode QT_CONV_FWD):
 *   dw[n][tap][k] += sum_pixels dy[pixel][n] * x[pixel moved by tap][k]     (f32)
 * replaces the conv/linear backward-weight ATen calls under loss.backward()
 * (Quadtree_from scratch/Quadtree_train.py:65).  `dw` must be zeroed (or hold the
 * running sum) by the caller: partial tiles are added with f32 atomics. */
int qt_conv2d_wgrad(const qt_conv_desc* desc, const void* dy, const void* x, float* dw, void* stream);
/* nn.Linear backward-weight (classifier.0 of the reference, Quadtree_from scratch/models.py:264-271): dw [out][in] f32 =
 * dy^T x over `rows` rows of dy [rows][out] and x [rows][in] (both of `dtype`, dense), WRITTEN -- where every tile of dw
 * has a single range of rows (always at rows <= 256) with plain stores, no zero fill and no atomics. */
int qt_linear_wgrad(int dtype, const void* dy, const void* x, float* dw, int rows, int out, int in, void* stream);
/* Same, with a caller-owned scratch buffer of qt_conv2d_wgrad_workspace_bytes(desc) bytes (0: this
 * shape does not use one).  With it the streaming kernel writes one partial filter per range of
 * positions with plain stores and a second kernel adds them to `dw` in a fixed order: no atomics,
 * bit-reproducible.  A NULL or too small workspace falls back to the atomic accumulation. */
size_t qt_conv2d_wgrad_workspace_bytes(const qt_conv_desc* desc);
int qt_conv2d_wgrad_ws(const qt_conv_desc* desc, const void* dy, const void* x, float* dw, void* workspace,
                       size_t workspace_bytes, void* stream);
/* The shapes with a workspace (bf16: 3x3 stride 1; and the stride-2 pair of a ResNet transition block, 3x3 / 2 pad 1 and
 * 1x1 / 2 on an even-sized map, csrc/conv_wgrad_s2.hip): the gradient is WRITTEN (not accumulated) in the
 * reference's OIHW layout by the kernel that sums the partial filters -- no [O][kh][kw][I] scratch,
 * no zero fill, no qt_unpack_conv_wgrad.  QT_ERR_UNSUPPORTED for every other shape. */
int qt_conv2d_wgrad_oihw(const qt_conv_desc* desc, const void* dy, const void* x, float* grad_oihw, void* workspace,
                         size_t workspace_bytes, void* stream);
/* The same, with the sum of the partial filters enqueued on `sum_stream` (behind the kernel through an event) instead of the
 * kernel's stream, which is then free for its next launch at once.  `workspace` must stay untouched until that sum has run:
 * the caller orders its next use of it behind sum_stream (for instance two workspaces used in turn).  The plan executor does
 * not use this entry point.  sum_stream NULL or == stream: qt_conv2d_wgrad_oihw. */
int qt_conv2d_wgrad_oihw_on(const qt_conv_desc* desc, const void* dy, const void* x, float* grad_oihw, void* workspace,
                            size_t workspace_bytes, void* stream, void* sum_stream);
/* bf16 3x3 / stride 1 / pad 1 weight gradients of images at least `min_width` wide take the
 * streaming kernel (csrc/conv_wgrad_patch.hip: one workgroup accumulates all nine taps of a
 * 64x64 channel tile while dY and X stream through LDS once).  0 = never, <0 = default (7: every stage of the
 * model).  Env QTCNN_WGRAD_PATCH_MIN_W. */
void qt_set_wgrad_patch_min_width(int min_width);
/* Which streaming kernel those shapes take: 3 = tile-resident (a tile of 128-256 padded positions + halo double
 * buffered in LDS, fragment reads two taps ahead of the MFMAs, source offsets from a table in LDS; default),
 * 0 / 2 = the round-1 ring kernel with one / two wave groups.  <0 = default; env QTCNN_WP_VARIANT. */
void qt_set_wgrad_patch_variant(int variant);
/* bf16 weight gradients of the stride-2 convolutions (3x3 / 2 pad 1, 1x1 / 2 pad 0, even map, channels % 64 == 0) on the
 * four parity planes of the input, tile-resident, all taps per workgroup, deterministic (csrc/conv_wgrad_s2.hip):
 * 1 = on (default), 0 = the generic kernel with float atomics, <0 = default.  Env QTCNN_WGRAD_S2. */
void qt_set_wgrad_s2(int on);

/* ------------------------------------------------------------------------
 * Layout packing (HBM-bound).
 * ------------------------------------------------------------------------ */
/* Packed stem input: [B][QT_STEM_PAD_H][QT_STEM_PAD_W][4] (3 zero rows/cols before,
 * 3 rows / 5 cols after, channel 3 zero) so that the 7x7/2 stem conv
 * (torchvision conv1, reached at Quadtree_from scratch/models.py:223) becomes 7
 * row taps of 32 contiguous elements: desc {kh=7,kw=1,stride=2,pad=0,k_per_tap=32,
 * src_pix_stride=4}.  Input contract: image [B,3,224,224] f32 NCHW
 * (Quadtree_from scratch/dataloader.py:72-91). */
#define QT_STEM_PAD_H 230
#define QT_STEM_PAD_W 232
int qt_pack_stem_input(int dtype, const float* image_nchw, void* dst, int batch, void* stream);
/* OIHW f32 master weights (reference state_dict layout) -> [O][kh][kw][I] (w_fwd)
 * and/or [I][kh][kw][O] (w_dgrad); either may be NULL.  Linear layers: kh=kw=1. */
int qt_pack_conv_weight(int dtype, const float* w_oihw, void* w_fwd, void* w_dgrad, int O, int I, int kh, int kw,
                        void* stream);
/* Every conv / linear weight of a model in one launch (LDS tile transposes): per item the same
 * result as qt_pack_conv_weight, or, with stride2_dgrad != 0 and k == 3, w_dgrad in the parity-class
 * layout of qt_pack_dgrad_s2 (stride2_dgrad = 1) or the merged layout of qt_pack_dgrad_s2_merged (= 2; only the
 * nine real taps are written: the zero slots of w_dgrad must have been zeroed once).  O and I must be multiples of
 * 32 (k = 3) or 64 (k = 1); at most 32 items.  Every pointer (masters, copies, and for the Adam form gradients and
 * moments) must be 16-byte aligned: the f32 streams move as float4. */
typedef struct qt_pack_item {
  const float* w_oihw;
  void* w_fwd;   /* nullable */
  void* w_dgrad; /* nullable */
  int O, I, k, stride2_dgrad;   /* stride2_dgrad: 0 stride 1; 1 parity classes (qt_pack_dgrad_s2); 2 merged, 4 slots
                                   (qt_pack_dgrad_s2_merged); 3 merged, FIVE slots per row (slot 4 belongs to the downsample);
                                   4 (k = 1): w_dgrad is that five-slot operand of the block's conv1 -- this item fills slot 4
                                   of the class-(0,0) rows: element ((i*5 + 4)*O + o) = w[o][i] (rows of the other classes
                                   keep the zeros qt_plan_init_workspace wrote) */
} qt_pack_item;
int qt_pack_weights_batched(int dtype, const qt_pack_item* items, int n, void* stream);
/* Adam with L2-in-gradient weight decay, torch.optim.Adam semantics without amsgrad / maximize
 * (the reference's optimizer, Quadtree_from scratch/Quadtree_train.py:45: lr 1e-4, weight_decay 1e-4):
 *   g = grad*grad_scale + wd*p;  m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g;
 *   p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps)                 all f32
 * qt_adam_multi: any list of tensors in one launch per 48 tensors.
 * qt_adam_pack_weights_batched: the same update INSIDE the one-launch weight packing, so the f32
 * masters, both moments and the packed operand copies are each touched once per step
 * (opt[j].param must be items[j].w_oihw).  `step` counts from 1; grad_scale 0 means 1. */
typedef struct qt_adam_desc {
  float lr, beta1, beta2, eps, weight_decay, grad_scale;
  int step;
} qt_adam_desc;
typedef struct qt_adam_item {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  long long numel;
} qt_adam_item;
int qt_adam_multi(const qt_adam_item* items, int n, const qt_adam_desc* adam, void* stream);
int qt_adam_pack_weights_batched(int dtype, const qt_pack_item* items, const qt_adam_item* opt, const qt_adam_desc* adam,
                                 int n, void* stream);
/* The same two calls with a second gradient factor that lives in DEVICE memory: the effective scale is
 * grad_scale * (*grad_scale_dev), applied where grad_scale is applied (one f32, 4-byte aligned, read by the kernel when
 * it runs, so a kernel earlier on the stream may produce it: qt_grad_norm_multi's clip_coef).  NULL: exactly
 * qt_adam_multi / qt_adam_pack_weights_batched, bit for bit. */
int qt_adam_multi_scaled(const qt_adam_item* items, int n, const qt_adam_desc* adam, const float* grad_scale_dev,
                         void* stream);
int qt_adam_pack_weights_batched_scaled(int dtype, const qt_pack_item* items, const qt_adam_item* opt,
                                        const qt_adam_desc* adam, const float* grad_scale_dev, int n, void* stream);
/* Global 2-norm of a list of f32 tensors and the clip coefficient of torch.nn.utils.clip_grad_norm_, without a host
 * round trip.  Of every item only `grad` (4-byte aligned, any numel >= 1) and `numel` are read.  Two deterministic
 * stages (fixed chunks, fixed summation order, no atomics): one sum of squares per 8192-element chunk into `workspace`
 * (at least qt_grad_norm_workspace_bytes of device memory; every slot used is written, nothing needs zeroing), then
 *   out2[0] = total_norm = sqrt(sum)
 *   out2[1] = clip_coef  = min(1, max_norm * (1 / (total_norm + 1e-6)))       all f32, torch's own evaluation order
 * in device memory.  A non-finite norm gives what torch gives (inf -> 0, NaN -> NaN).  One launch per 48 tensors plus
 * one.  max_norm <= 0 or NaN: QT_ERR_INVALID_ARG.  The workspace size depends on the pointers' alignment as well as on
 * the element counts: ask for it with the list that is passed (returns 0 and sets the error text for a bad list). */
size_t qt_grad_norm_workspace_bytes(const qt_adam_item* items, int n);
int qt_grad_norm_multi(const qt_adam_item* items, int n, float max_norm, void* workspace, size_t workspace_bytes,
                       float* out2, void* stream);
/* Loss head: replaces nn.CrossEntropyLoss()(outputs, labels) and its backward (3dcnn/train_3D_Quadtree_cnn_model.py:108-111,
 * every other trainer alike), FocalLoss (3dcnn/models.py:8-47) and the per-step bookkeeping of the trainers
 * (loss.item(), torch.max(outputs.data, 1), (predicted == labels).sum().item(): :127-137) without a host round trip.
 * logits: f32 [rows][C], row stride ld >= C elements (views are fine); labels: int64 [rows]; 1 <= C <= 1024, rows >= 1.
 * QT_ERR_UNSUPPORTED for another dtype, C > 1024 and 0 < gamma < 1; QT_ERR_INVALID_ARG for every other bad argument.
 * With p = softmax(z), w = class_weight (NULL: all ones), y = label:
 *   QT_LOSS_CROSS_ENTROPY  loss_i = (1-eps) w[y] (-log p_y) + (eps/C) sum_c w[c] (-log p_c); a row whose label equals
 *                          ignore_index contributes 0 and gets a zero gradient; MEAN divides by the sum of w[y] over the
 *                          other rows (no such row: NaN) -- torch.nn.functional.cross_entropy with class-index targets;
 *   QT_LOSS_FOCAL          loss_i = -w[y] (1-p_y)^gamma log p_y, w = the reference's alpha; MEAN divides by rows;
 *                          ignore_index and label_smoothing are not read; gamma = 0 or gamma >= 1.
 * A label outside [0, C) that is not an ignored one cannot be refused by the host.  The kernels never index with it: such
 * a row's loss is NaN, which makes the reduced loss and (MEAN / SUM) every gradient NaN; with NONE only that row's loss
 * and gradient row are NaN.  Its pred entry is still the argmax.
 * Both calls enqueue on `stream` only: no allocation, no atomics, no zero fill, no host synchronisation, the same bits on
 * every run.  One launch each while the rows fit one workgroup (256 rows for C <= 16, 16 for C <= 64, else 4); above
 * that the forward is per-workgroup partial sums in `workspace` (qt_loss_workspace_bytes; 0 = none needed, NULL is fine)
 * plus a one-workgroup finalize that adds them in double in a fixed order.
 * qt_loss_forward writes
 *   loss       one f32 (MEAN / SUM) or [rows] (NONE)
 *   row_state  [rows][2] f32 {max logit, log(sum exp(z - max))} for the backward; NULL when no backward follows
 *   stats      double[3] {sum of loss_i, denominator the reduction divides by (1 for SUM / NONE), #(pred == label)}
 *   pred       int64 [rows] argmax as torch.max(outputs, 1) on the CPU gives it: the first index wins a tie, a NaN logit
 *              wins its row; or NULL
 *   meter      double[4] {loss_sum, samples, correct, skipped_steps} owned by the caller, updated by one thread after the
 *              reduction, or NULL.  Reduced loss finite: loss_sum += loss * rows (MEAN) or += loss (SUM; NONE: the sum of
 *              loss_i), samples += rows, correct += stats[2].  Otherwise skipped_steps += 1 and nothing else.
 * qt_loss_backward reads the same logits / labels, row_state and stats, and the upstream gradient grad_out from DEVICE
 * memory (one f32; [rows] for NONE), and writes dlogits [rows][ld_d] (columns >= C untouched):
 *   cross-entropy  [(1-eps) w[y] (p_k - [k == y]) + (eps/C) (p_k sum_c w[c] - w[k])] * grad_out / stats[1]
 *   focal          w[y] [(1-p_y)^gamma - gamma p_y (1-p_y)^(gamma-1) log p_y] (p_k - [k == y]) * grad_out / stats[1] */
enum { QT_LOSS_CROSS_ENTROPY = 0, QT_LOSS_FOCAL = 1 };
enum { QT_LOSS_REDUCE_MEAN = 0, QT_LOSS_REDUCE_SUM = 1, QT_LOSS_REDUCE_NONE = 2 };
typedef struct qt_loss_desc {
  int dtype;                  /* of the logits: QT_F32 */
  int kind, reduction;
  long long ignore_index;     /* torch's default: -100 */
  float label_smoothing;      /* eps in [0, 1] */
  float gamma;
  const float* class_weight;  /* device, [C], or NULL */
} qt_loss_desc;
size_t qt_loss_workspace_bytes(long long rows, int C);
int qt_loss_forward(const qt_loss_desc* desc, const float* logits, long long ld, const long long* labels, long long rows, int C,
                    float* loss, float* row_state, double* stats, long long* pred, double* meter, void* workspace,
                    size_t workspace_bytes, void* stream);
int qt_loss_backward(const qt_loss_desc* desc, const float* logits, long long ld, const long long* labels, long long rows, int C,
                     const float* row_state, const double* stats, const float* grad_out, float* dlogits, long long ld_d,
                     void* stream);
/* Frame preprocessing: what the reference's loaders do per image on the host (RandomResizedCrop / Resize -> ToTensor ->
 * Normalize, RandomHorizontalFlip; experiment/test_on_video_cnn.py:228-254, cnn+lstm/prepare_sequential_dataset.py:30-33,
 * 3dcnn/dataloaders.py:99-102), from decoded uint8 frames to the f32 [batch][3][out_h][out_w] tensor the models take, in one
 * launch.  A clip [B][T][H][W][3] -> [B][T][3][h][w] is the same call with batch = B * T.
 * Per image: crop `box`, resize the crop to out_h x out_w with torch's antialiased bilinear rule
 * (interpolate(mode='bilinear', antialias=True); PIL's BILINEAR resize without its uint8 rounding between the two passes:
 * at most one grey level away), mirror the columns where flips[b] != 0, then (v / 255 - mean[c]) * inv_std[c].
 * For an axis of crop length `in` and output length `out`: scale = in / out, support = max(scale, 1), center = scale (i + 0.5),
 * taps j in [max(floor(center - support + 0.5), 0), min(floor(center + support + 0.5), in)) relative to the crop, raw weight
 * max(0, 1 - |(j - center + 0.5) / support|), divided by their sum; no pixel outside the box is read.
 * boxes and flips are read on the device: nothing is synchronised, nothing allocated, no atomics, no intermediate in HBM,
 * the same bits on every run.  A box that is not inside its frame (or has height < 1 or width < 1) cannot be refused by the
 * host: that image's output is all NaN, nothing of its frame is read, the other images are unaffected.
 * QT_ERR_INVALID_ARG (before any device call) for non-positive sizes, strides smaller than a row / an image, null or
 * misaligned pointers; QT_ERR_UNSUPPORTED (before any launch) for a frame more than 24 x the output on an axis (the
 * downscale limit: the taps of a tile must fit one workgroup's LDS) and for sizes above 2^22. */
typedef struct qt_preprocess_desc {
  int batch, src_h, src_w;          /* frames are uint8 HWC, 3 channels, interleaved */
  long long src_row_stride;         /* bytes, >= 3*src_w */
  long long src_image_stride;       /* bytes, >= src_h*src_row_stride */
  int out_h, out_w;
  int bgr;                          /* 1: source channel order is B,G,R (cv2 frames); output is always R,G,B planes */
  float mean[3], inv_std[3];        /* per output channel (R,G,B) */
} qt_preprocess_desc;
int qt_preprocess_u8(const qt_preprocess_desc* desc, const unsigned char* src,
                     const int* boxes,          /* device, [batch][4] = top,left,height,width; NULL = whole frame */
                     const unsigned char* flips,/* device, [batch], nonzero = mirror left-right; NULL = none */
                     float* dst, long long dst_image_stride /* floats, >= 3*out_h*out_w */, void* stream);
/* Training augmentations: the middle of the reference's training transform (Quadtree_from scratch/dataloader.py:29-37,
 * resnet/dataloader.py:32-40), ColorJitter -> RandomRotation -> GaussianBlur -> Normalize, on f32 [batch][3][h][w] planes with
 * values in [0, 1] (what qt_preprocess_u8 writes with mean 0, inv_std 1), by the rule of torchvision's float-tensor path
 * (without PIL's uint8 rounding between the steps: about a grey level apart per stage).
 * params: device, [batch][QT_AUGMENT_PARAMS] f32, read on the device only:
 *   0-3   brightness, contrast, saturation factor, hue shift
 *   4-7   the order: four slots, each -1 (skip) or an op id 0 = brightness, 1 = contrast, 2 = saturation, 3 = hue; no id twice
 *   8, 9  cos, sin of the rotation angle (counter-clockwise); (1, 0) = no rotation
 *   10    blur sigma (> 0 when a blur kernel is set)       11  reserved, 0
 * A malformed row (a non-finite entry, a slot outside {-1, 0, 1, 2, 3}, a repeated id, sigma <= 0 while blur is on, op 1 while
 * use_contrast == 0) makes that image's output all NaN; the other images are unaffected.
 * With gray = 0.2989 r + 0.587 g + 0.114 b and blend(a, b, f) = clamp(f a + (1 - f) b, 0, 1), in the slots' order:
 *   brightness blend(img, 0, f); contrast blend(img, m, f), m = mean of gray over the whole image as it stands when the op is
 *   reached; saturation blend(img, gray(img), f); hue RGB -> HSV, h = (h + shift) mod 1, HSV -> RGB:
 *     v = maxc, s = (maxc - minc) / maxc, rc = (maxc - r) / (maxc - minc) (g, b likewise; a zero divisor is replaced by 1),
 *     h = [maxc == r] (bc - gc) + [maxc == g, != r] (2 + rc - bc) + [maxc != g, != r] (4 + gc - rc), h = fmod(h / 6 + 1, 1);
 *     i = floor(6 h), f = 6 h - i, p = clamp(v (1 - s)), q = clamp(v (1 - s f)), t = clamp(v (1 - s (1 - f))),
 *     (r, g, b) = (v,t,p) (q,v,p) (p,v,t) (p,q,v) (t,p,v) (v,p,q) for i mod 6 = 0 .. 5.
 * Rotation: nearest neighbour about the image centre, same size, fill 0 (not jittered): output pixel (i, j) has
 *   x = j + 0.5 - w/2, y = i + 0.5 - h/2 and reads column round(cos x - sin y + w/2 - 0.5), row round(sin x + cos y + h/2 - 0.5).
 * Blur: separable, blur_kx taps along a row and blur_ky along a column, weight exp(-0.5 (d / sigma)^2) / sum for offset d, the
 *   border reflected without repeating the edge pixel (index -1 reads 1); (1, 1) = no blur.  Then (v - mean[c]) * inv_std[c].
 * clamp keeps a NaN (torch.clamp): a NaN input pixel is NaN wherever the rule carries it.
 * No intermediate image in HBM, no atomics, no zero fill, no host synchronisation, the same bits on every run.  With
 * use_contrast == 1 a first launch writes QT_AUGMENT_PARTS partial sums per image into the workspace
 * (qt_augment_workspace_bytes; 0 and NULL when use_contrast == 0, the caller's promise that no row names op 1).
 * QT_ERR_INVALID_ARG (before any device call) for non-positive sizes, a blur size that is even or above 15, an image the blur
 * reflects beyond (needs w > blur_kx / 2, h > blur_ky / 2), strides below 3*h*w, null or misaligned pointers, a workspace that
 * is too small, source and destination that overlap (rotation and blur gather); QT_ERR_UNSUPPORTED for sizes above 2^22. */
#define QT_AUGMENT_PARAMS 12
#define QT_AUGMENT_PARTS 16
typedef struct qt_augment_desc {
  int batch, h, w;
  long long src_image_stride;       /* floats, >= 3*h*w */
  long long dst_image_stride;       /* floats, >= 3*h*w */
  int blur_kx, blur_ky;             /* odd, <= 15 */
  float mean[3], inv_std[3];
  int use_contrast;
} qt_augment_desc;
size_t qt_augment_workspace_bytes(int batch, int use_contrast);
int qt_augment_f32(const qt_augment_desc* desc, const float* src, const float* params, float* dst, void* workspace,
                   size_t workspace_bytes, void* stream);
/* Grad-CAM: the heat map of the reference's three Grad-CAM scripts (resnet/grad_cam_analysis.py:306-343,
 * grad_cam/5_grad_cam_visualizer.py:220-275, Quadtree_from scratch/grad_cam.py:70-96) for a whole batch, from the two hook
 * tensors to uint8 overlays, without a host read.
 * qt_gradcam_map.  act, grad: f32, contiguous [batch][C][P], the hooked layer's output and the gradient of the class score
 * with respect to it; P = the number of positions (h w for base_cnn.layer4, t h w for Quadtree3DCNN.conv3d_final_features).
 * cam: f32 [batch][P]; peak: f32 [batch].  Per image, on its own:
 *   w_c = (sum_p grad[c][p]) / P;  s_p = sum_c w_c act[c][p];  r_p = max(s_p, 0);  peak = max_p r_p;
 *   cam_p = r_p / peak, and cam_p = 0 for every p when peak == 0.
 * (grad_cam_analysis.py:306-324 image by image.  Quadtree_from scratch/grad_cam.py:84 takes the mean over the channels where
 * this takes the sum: the normalised map is the same.  That script divides by a zero peak and gets NaN; here such a map
 * is all zeros, as in the other two scripts.)  Both maxima carry a NaN, and w_c act[c][p] is NaN where either factor is:
 * an image with a NaN anywhere in its act or grad gets an all-NaN map and a NaN peak; the other images are not touched
 * by it.  Any C >= 1; 1 <= P <= QT_GRADCAM_MAX_POSITIONS, above that QT_ERR_UNSUPPORTED before any launch.
 * C <= 32: one launch, no workspace (qt_gradcam_workspace_bytes returns 0, NULL is fine).  Otherwise one workgroup per
 * image and 32-channel chunk writes its part of s_p to the workspace ([batch][ceil(C / 32)][P] f32, every slot used is
 * written) and a second launch adds the chunks in ascending order.  Every summation order depends on (C, P) only: no
 * atomics, no zero fill, no host synchronisation, the same bits on every run and for an image alone or in a batch.
 * qt_gradcam_overlay_u8.  cam: f32 [batch][h][w]; frames, out: uint8 [batch][H][W][3], contiguous; lut: uint8 [256][3] in
 * DEVICE memory, in the frames' channel order; heat: f32 [batch][H][W] or NULL; index: uint8 [batch][H][W] or NULL.
 * Per output pixel (y, x):
 *   v    = the map sampled bilinearly with pixel centres at half-integers: f_x = (x + 0.5) (w / W) - 0.5, taps floor(f_x) and
 *          floor(f_x) + 1 with weights 1 - t and t, t = f_x - floor(f_x), a tap outside the map replaced by the nearest one
 *          inside; rows likewise.  (The rule cv2.resize documents for INTER_LINEAR; bit equality with it is not claimed.)
 *   idx  = v > 0 ? min(255, int(255 v)) : 0, so a NaN map value gives idx 0 (and NaN in heat);
 *   out  = uint8(floor(alpha lut[idx][c] + (1 - alpha) frames[c])) per channel: np.uint8(255 * heatmap) and
 *          np.uint8(heatmap * alpha + image * (1 - alpha)) of visualize_cam; heat = v, index = idx.
 * One launch, 16-byte accesses wherever frames and out have the same address modulo 16 (any address works); nothing is
 * read or written outside the stated extents; the same bits on every run.  out may be frames itself; no other overlap.
 * QT_ERR_INVALID_ARG (before any device call) for non-positive sizes, alpha outside [0, 1], null or misaligned pointers,
 * a workspace that is too small; QT_ERR_UNSUPPORTED for overlay sizes above 2^22. */
#define QT_GRADCAM_MAX_POSITIONS 4096
size_t qt_gradcam_workspace_bytes(int batch, int C, int P);
int qt_gradcam_map(const float* act, const float* grad, int batch, int C, int P, float* cam, float* peak, void* workspace,
                   size_t workspace_bytes, void* stream);
int qt_gradcam_overlay_u8(const float* cam, int h, int w, const unsigned char* frames, int batch, int H, int W,
                          const unsigned char* lut, float alpha, unsigned char* out, float* heat, unsigned char* index,
                          void* stream);
/* The pose vector: the 47 numerical features the models take beside the image, from 33 MediaPipe landmarks (source A; the
 * rule of experiment/test_on_video_cnn.py:126-202) or from the stored raw vectors (source B), followed by the loaders' NaN
 * imputation (test_on_video_cnn.py:261, Quadtree_from scratch/dataloader.py:84-88, 3dcnn/dataloaders.py:119-139), in one
 * launch.  Exactly one of `landmarks` and `raw` is given; out: f32 [rows][47].
 * Source A.  landmarks: f32 [rows][33][4] = x, y, z, visibility per landmark, 16-byte aligned; detected: uint8 [rows] or
 * NULL (every row detected).  With p_j = (x, y, z) of landmark j and all arithmetic in f32:
 *   0-32   visibility of landmark j.
 *   33-40  the angle at b of (a, b, c) in degrees for (11,13,15) (12,14,16) (23,11,13) (24,12,14) (23,25,27) (24,26,28)
 *          (11,23,25) (12,24,26): ba = p_a - p_b, bc = p_c - p_b, deg(atan2(|ba x bc|, ba . bc)); NaN when ba or bc is the
 *          zero vector.
 *   41     t = (p11 + p12) / 2 - (p23 + p24) / 2 in x, y;  d = |deg(pi/2 - atan2(t.y, t.x))|;  d > 180: d = 360 - d.
 *   42     d = |deg(atan2(p12 - p11)) - deg(atan2(p24 - p23))| in x, y, folded at 180 likewise.
 *   43-45  |p15 - p16|, |p27 - p28|, |p15 - p23| (3-D) divided by s:  sw = |p11 - p12|, hw = |p23 - p24|;  s = (sw + hw) / 2
 *          when sw > 0 and hw > 0, else 1;  s == 0: s = 1;  unless s > 0.05 all three are NaN.
 *   46     over those of landmarks 11, 12, 23, 24 whose visibility is > 0.65: var(x) / var(y), population variances in
 *          two passes (the mean, then the squared deviations); NaN with fewer than two of them or when var(y) == 0.
 * A row with detected == 0 gives 0.0 in columns 0-32 and NaN in 33-46.  A NaN coordinate goes by IEEE rules into the
 * features that read it (a comparison with it is false: a NaN shoulder gives s = 1); a NaN visibility is not visible.
 * The reference takes the angle as arccos(ba . bc / (|ba| |bc|)) in float64; in f32 that form loses half its digits near
 * 0 and 180 degrees, atan2 does not, and it is the same angle.  Two of the reference's behaviours differ: on exactly
 * collinear points numpy's arccos returns NaN when rounding pushes the cosine past +-1, the rule here gives 0 or 180; a
 * zero-length limb (0 / 0 there) is NaN in both.
 * Source B.  raw: f32 [rows][47], NaNs included.  out == raw is allowed (every element is read and written by the same
 * thread); no other overlap.
 * Imputation (desc->mode), applied to either source's values v in the same launch; label = labels[row / rows_per_label]
 * (int64, device; rows_per_label must divide rows: one label per sequence of a [B][T] batch), means, stds: f32
 * [num_classes][47], device:
 *   QT_POSE_RAW          v (NaNs stay)
 *   QT_POSE_ZERO         NaN -> 0
 *   QT_POSE_CLASS_MEAN   NaN -> means[label][f]
 *   QT_POSE_STANDARDIZE  NaN -> means[label][f], then (v - means[label][f]) / stds[label][f]; 0 where stds[label][f] < 1e-6f
 * In the last two modes a label outside [0, num_classes) makes that row all NaN: only the device sees the label, nothing
 * is indexed with it, the other rows are unaffected.  (The reference's loaders fall back to zeros for an unknown class,
 * silently; that is not reproduced.)  labels, means, stds are not read in the first two modes.
 * No atomics, no zero fill, no workspace, no host synchronisation; the same bits on every run and for a row alone or
 * inside a batch.
 * QT_ERR_INVALID_ARG (before any device call) for non-positive sizes, both or neither source, `detected` with source B,
 * null or misaligned pointers, an unknown mode, a mode without the labels / tables it needs, rows_per_label that does not
 * divide rows; QT_ERR_UNSUPPORTED for more than 2^22 rows. */
#define QT_POSE_LANDMARKS 33
#define QT_POSE_FEATURES 47
enum { QT_POSE_RAW = 0, QT_POSE_ZERO = 1, QT_POSE_CLASS_MEAN = 2, QT_POSE_STANDARDIZE = 3 };
typedef struct qt_pose_desc {
  long long rows;
  int mode;                         /* QT_POSE_* */
  int rows_per_label;               /* >= 1; read in the two class modes only */
  int num_classes;                  /* K of means / stds; read in the two class modes only */
} qt_pose_desc;
int qt_pose_features(const qt_pose_desc* desc, const float* landmarks, const unsigned char* detected, const float* raw,
                     const long long* labels, const float* means, const float* stds, float* out, void* stream);
/* Sequence pose features: the 443 columns per frame that sqn process/processing_image_sequence.py:96-247
 * (calculate_all_features, driven per clip by the loop at :374-441) writes and create_sequential_dataset.py:179-181 stores as a
 * sequence's features.npy, followed by the CNN+LSTM loader's NaN -> 0 (cnn+lstm/dataloader.py:64-65), in one launch.  Unlike
 * the 47-vector a frame depends on earlier frames of its clip.
 * landmarks: f32 [batch][frames][33][4] = x, y, z, visibility, 16-byte aligned; detected: uint8 [batch][frames] or NULL (a
 * pose in every frame); sizes: int32 [batch][2] = (W, H) of each clip's frames, device, or NULL for desc->width / height;
 * out: f32 [batch][frames][443].  All arithmetic is f32.  q_j = (x_j W, y_j H, z_j W) is the pixel position of landmark j.
 * A landmark is visible iff visibility > 0.65f.  The reference tests `visibility < 0.65` (not visible) in one helper and
 * `visibility > 0.65` (visible) elsewhere, both against a double; for an f32 v, double(v) < 0.65 <=> v <= 0.65f and
 * double(v) > 0.65 <=> v > 0.65f (0.65 is no f32: it lies between 0.65f and the next f32 above), so the one predicate
 * reproduces both.  A NaN
 * visibility is not visible (the reference's `<` gate lets a NaN through; that is not reproduced).
 *   4j .. 4j+3  (0-131)    x, y, z, visibility of landmark j as given.
 *   132-141   the angle at b of (a, b, c) in degrees over q for (11,13,15) (12,14,16) (13,11,23) (14,12,24) (23,25,27)
 *             (24,26,28) (11,23,25) (12,24,26) (0,11,23) (11,12,23): NaN unless a, b, c are visible, else
 *             deg(atan2(|ba x bc|, ba . bc)) with ba = q_a - q_b, bc = q_c - q_b, which is 0 when ba or bc is the zero
 *             vector (the reference returns 0.0 there).  The reference's arccos(clip(ba . bc / (|ba| |bc|))) is the same
 *             angle; in f32 it loses half its digits near 0 and 180 degrees, atan2 does not (as for qt_pose_features).
 *   142-144   |q15 - q16|, |q27 - q28|, |q15 - q23| divided by s, NaN unless both landmarks are visible.  sw = |q11 - q12|
 *             if 11 and 12 are visible, else 0; hw = |q23 - q24| likewise; s = sw if sw > 0.05f W, else hw if
 *             hw > 0.05f W, else H / 3.
 *   145+3j .. (145-243)    (x, y, z)_j - m, NaN if landmark j is not visible; m = ((x, y, z)_23 + (x, y, z)_24) * 0.5f if 23
 *             and 24 are visible, else (0.5, 0.5, 0).
 *   244+6j .. (244-441)    v = q_j - q'_j, then a = v - (q'_j - q''_j), where ' and '' are the most recent and the second
 *             most recent DETECTED frames before this one in the clip (undetected frames do not enter the history:
 *             :375, :410-416).  All six are NaN unless landmark j is visible in all three frames, and when fewer than two
 *             such frames exist (the reference leaves the velocity NaN too then).  All three positions use this clip's
 *             (W, H).
 *   442       over the visible ones of landmarks 11, 12, 23, 24: (var(x) + 1e-6f) / (var(y) + 1e-6f), population variances
 *             in two passes (the mean, then the squared deviations); NaN with fewer than two.
 * A frame with detected == 0 is 443 NaNs (the reference's dummy dict has mis-spelt keys and pandas leaves the real columns
 * NaN); its landmark values are not used.  A non-positive W or H in device `sizes` makes that clip's rows NaN (only the
 * device sees it); the history is carried as usual.  Then desc->mode: QT_POSE_RAW (NaNs stay) or QT_POSE_ZERO (NaN -> 0);
 * the two class-table modes do not exist for these columns.
 * History across calls (a live loop hands frames over in chunks).  hist_in: f32 [batch][2][33][4], the landmarks of the last
 * two detected frames before this call's first frame, slot 0 the most recent, 16-byte aligned, with hist_count_in: uint8
 * [batch], how many slots hold a frame (0, 1, 2; more counts as 2); both NULL: every clip starts empty.  hist_out /
 * hist_count_out (both or neither) receive the same state after the last frame of the call; slots beyond the count are
 * written as zeros.  hist_out must not overlap hist_in, nor hist_count_out hist_count_in (other workgroups still read them):
 * a caller swaps two buffers.  A clip processed in any split into consecutive calls gives the same bits as one call.
 * One launch, no atomics, no zero fill, no workspace, no host synchronisation; the same bits on every run and for a clip
 * alone or inside a batch.  Inputs are never written.
 * QT_ERR_INVALID_ARG (before any device call) for non-positive batch or frames, null or misaligned pointers (landmarks and
 * the histories 16 bytes, out and sizes 4), half a history pair, overlapping histories, a mode other than RAW and ZERO, a
 * non-positive desc->width / height when sizes is NULL; QT_ERR_UNSUPPORTED for more than 2^22 frames in all. */
#define QT_POSE_SEQ_FEATURES 443
typedef struct qt_pose_seq_desc {
  int batch;                        /* clips */
  int frames;                       /* frames per clip in this call */
  int width, height;                /* frame size of every clip; read when `sizes` is NULL */
  int mode;                         /* QT_POSE_RAW or QT_POSE_ZERO */
} qt_pose_seq_desc;
int qt_pose_sequence_features(const qt_pose_seq_desc* desc, const float* landmarks, const unsigned char* detected,
                              const int* sizes, const float* hist_in, const unsigned char* hist_count_in, float* hist_out,
                              unsigned char* hist_count_out, float* out, void* stream);
/* Sequence windows: the step between labelled clips and the [B][T][...] samples of the sequence models, with every clip held
 * on the device once instead of one stored copy per window (sqn process/create_sequential_dataset.py:154-205 copies 10 frames
 * per window at stride 1; cnn+lstm/prepare_sequential_dataset.py:36-112 stores every window as T normalised f32 frames).
 * Three entry points: which windows there are (qt_seq_windows_plan), a batch of windows of any per-frame array
 * (qt_seq_gather_rows), a batch of windows of f32 pose rows with the loaders' imputation (qt_seq_gather_features).
 *
 * qt_seq_windows_plan.  labels: int64 [frames], device: the frames of all clips one after the other, each clip in temporal
 * order; clip_offsets: int32 [clips + 1], device, ascending from 0 to frames (clip c is frames clip_offsets[c] ..
 * clip_offsets[c + 1] - 1; an empty clip is allowed).  Candidate starts are clip_offsets[c] + i for i = 0, stride, 2 stride, ...
 * while i + seq_len <= the clip's length: a window never crosses a clip boundary, a clip shorter than seq_len gives none.
 * desc->rule decides which candidates are kept and their label:
 *   QT_SEQ_LABEL_UNIFORM  (create_sequential_dataset.py:164-171) kept iff the window's seq_len labels are all equal and lie in
 *                         [0, num_classes); the label is that value.
 *   QT_SEQ_LABEL_LAST     (prepare_sequential_dataset.py:46-62) the label is the last frame's; kept iff it lies in
 *                         [0, num_classes).  The other frames' labels are not looked at.
 * starts: int32 [capacity], the kept starts in ascending frame order (the reference's order: clips in order, i ascending);
 * window_labels: int64 [capacity], their labels; count: int32 [1], the number of kept windows.  When it exceeds capacity only
 * the first capacity starts and labels are written and count still holds the total; elements at and behind count are not
 * written.  (Capacity never needs to exceed the number of candidates, sum over clips of max(0, (n_c - seq_len) / stride + 1).)
 * The only notion of "no label" is a value outside [0, num_classes).  The reference removes the frames that have no label
 * from its table BEFORE it windows (create_sequential_dataset.py:125-127), so its windows run over the remaining frames and
 * may bridge the gap; that filter is the caller's, applied to the labels, the offsets and the per-frame arrays alike before
 * this call.
 * Three launches on `stream` (counts per workgroup, an exclusive scan of the counts by one workgroup, the scatter); the
 * partial counts live in `workspace` (qt_seq_windows_workspace_bytes, 4-byte aligned; every slot used is written, nothing
 * needs zeroing).  No workgroup waits for another inside a launch, no atomics, no host synchronisation; the same bits on
 * every run.  clip_offsets is read at indices 0 .. clips and labels at 0 .. frames - 1 only, whatever the offsets hold: a
 * clip's end is cut at frames, and offsets that do not ascend give fewer windows, never a read outside an array.
 * QT_ERR_INVALID_ARG (before any device call) for a null desc, non-positive frames, clips, num_classes, capacity or stride,
 * seq_len outside 1 .. 64, an unknown rule, null or misaligned pointers (8 bytes for the int64 arrays, 4 for the others), a
 * workspace that is too small; QT_ERR_UNSUPPORTED for more than 2^22 frames.  qt_seq_windows_workspace_bytes returns 0 for
 * a descriptor the call would refuse.
 *
 * qt_seq_gather_rows.  dst[b][t][:] = src[starts[b] + t][:] for b < windows, t < seq_len; rows of row_bytes bytes (any
 * value >= 1), src of src_rows rows, starts: int32 [windows], device (the loader's plan.starts[idx]; duplicates are fine).
 * A window is one contiguous run of seq_len * row_bytes bytes; source and destination run need not agree modulo 16: units of
 * 16 bytes where they do, of 4 bytes where they agree modulo 4, single bytes otherwise, with single bytes up to the
 * destination's first boundary and behind the last whole unit.  src and dst need no alignment.  A start outside
 * [0, src_rows - seq_len] makes that window's seq_len * row_bytes bytes 0xFF (NaN as f32 and bf16, 255 as a byte): only the
 * device sees the value, nothing is read for it, the other windows are unaffected.  One launch, 64-bit byte offsets, no
 * atomics, no workspace, no host synchronisation; nothing outside src is read, src is not written.
 * QT_ERR_INVALID_ARG (before any device call) for a null desc, non-positive src_rows, row_bytes or windows, seq_len outside
 * 1 .. 64, null pointers, misaligned starts, src and dst that overlap; QT_ERR_UNSUPPORTED for src_rows >= 2^31, row_bytes above
 * 2^34 or more workgroups than one launch takes.
 *
 * qt_seq_gather_features.  The same gather for f32 rows of desc->features columns (1 .. 1024; 47 and 443 are in use), out:
 * f32 [windows][seq_len][features], with the imputation of qt_pose_features applied as an element is stored, by desc->mode
 * and ONE label per window, label = window_labels[b] (int64 [windows], device; 3dcnn/dataloaders.py:186-207 uses the
 * sequence's label for every frame); means, stds: f32 [num_classes][features], device:
 *   QT_POSE_RAW          v (NaNs stay); the same bytes as qt_seq_gather_rows
 *   QT_POSE_ZERO         NaN -> 0
 *   QT_POSE_CLASS_MEAN   NaN -> means[label][f]
 *   QT_POSE_STANDARDIZE  NaN -> means[label][f], then (v - means[label][f]) / stds[label][f] in f32; 0 where
 *                        stds[label][f] < 1e-6f
 * which for features == 47 are the bits of qt_pose_features on the gathered rows with rows_per_label = seq_len.  In the last
 * two modes a label outside [0, num_classes) makes that window NaN (nothing is indexed with it); a start outside
 * [0, src_rows - seq_len] makes it 0xFF bytes (a NaN) in every mode.  window_labels, means, stds are not read in the first two
 * modes.  One launch, no atomics, no workspace, no host synchronisation; the same bits on every run.
 * QT_ERR_INVALID_ARG (before any device call) for a null desc, non-positive src_rows or windows, features outside 1 .. 1024,
 * seq_len outside 1 .. 64, an unknown mode, a class mode without the labels / tables it needs, null or misaligned pointers (4
 * bytes for f32 and int32, 8 for window_labels), rows and output that overlap; QT_ERR_UNSUPPORTED for src_rows >= 2^31. */
enum { QT_SEQ_LABEL_UNIFORM = 0, QT_SEQ_LABEL_LAST = 1 };
typedef struct qt_seq_windows_desc {
  int frames;                       /* frames of all clips together, <= 2^22 */
  int clips;
  int seq_len;                      /* 1 .. 64 */
  int stride;                       /* >= 1 */
  int num_classes;
  int capacity;                     /* elements of starts / window_labels */
  int rule;                         /* QT_SEQ_LABEL_* */
} qt_seq_windows_desc;
size_t qt_seq_windows_workspace_bytes(const qt_seq_windows_desc* desc);
int qt_seq_windows_plan(const qt_seq_windows_desc* desc, const long long* labels, const int* clip_offsets, int* starts,
                        long long* window_labels, int* count, void* workspace, size_t workspace_bytes, void* stream);
typedef struct qt_seq_gather_desc {
  long long src_rows;
  long long row_bytes;
  int windows;
  int seq_len;
} qt_seq_gather_desc;
int qt_seq_gather_rows(const qt_seq_gather_desc* desc, const void* src, const int* starts, void* dst, void* stream);
typedef struct qt_seq_features_desc {
  long long src_rows;
  int features;                     /* 1 .. 1024 */
  int windows;
  int seq_len;
  int mode;                         /* QT_POSE_* */
  int num_classes;                  /* K of means / stds; read in the two class modes only */
} qt_seq_features_desc;
int qt_seq_gather_features(const qt_seq_features_desc* desc, const float* raw, const int* starts, const long long* window_labels,
                           const float* means, const float* stds, float* out, void* stream);
/* Evaluation report: the confusion matrix, precision / recall / F1, R^2 and the per-frame softmax confidence that the
 * reference's scripts end on (comparative analysis/analysis.py:60-109, 3dcnn/train_3D_Quadtree_cnn_model.py:248,
 * VIT/fact_model_train.py:153, experiment/test_on_video_cnn.py:274-278), without the two host copies per batch and
 * without scikit-learn.  The data is additive integer counts that stay in device memory for a whole evaluation:
 *   state   u64 [C*C + 4] = { cm[label * C + pred] ..., rows counted, rows ignored, rows invalid, update calls }
 * (qt_metrics_state_bytes = 8 (C*C + 4)).  The caller zeroes it once; qt_metrics_update only ever adds to it, so the
 * states of several streams, devices or ranks add up to the state of their union.  1 <= C <= QT_METRICS_MAX_CLASSES,
 * 1 <= rows <= 2^22 per call; both size queries return 0 for a C outside the range.
 * qt_metrics_update, one launch per batch.  Exactly one of `logits` and `pred_in`:
 *   logits     f32 [rows][C], row stride ld >= C elements.  pred = torch.max(logits, 1)'s index by the total order of the
 *              loss head (a NaN beats every number, then the larger value, then the lower index): bit-identical to the
 *              `pred` of qt_loss_forward on the same buffer.  With m = logits[pred], all in f32:
 *                e_k = expf(z_k - m), s = sum_k e_k, p_k = e_k / s
 *              probs [rows][ld_probs] receives p (columns >= C untouched), confidence [rows] receives p[pred] (the very
 *              f32 stored to probs[pred]), pred_out [rows] receives pred (int64); each may be NULL.  A row with a NaN or
 *              +inf logit (or all -inf) is NaN in every column and in confidence, as torch.softmax gives on the CPU.
 *              Padding columns of the logits are not read into anything.
 *   pred_in    int64 [rows], e.g. the `pred` output of qt_loss_forward: counting only (no probs / confidence / pred_out).
 * Counting, when `labels` (int64 [rows]) and `state` are given (both or neither; without them the call only produces
 * probs / confidence / pred_out): per row, in this order,
 *   label == desc->ignore_index                                      -> rows ignored += 1
 *   label outside [0, C), or a given prediction outside [0, C)        -> rows invalid += 1 (nothing is indexed with it)
 *   otherwise                                                         -> cm[label * C + pred] += 1, rows counted += 1
 * and update calls += 1 once per call.  Every add is an integer atomic, so the counts are exact in any order of
 * execution: C <= 64 counts in a per-workgroup u32 histogram in LDS and adds each non-zero cell to the state with one
 * 64-bit atomic; above that every counted row is one 64-bit atomic.  No allocation, no host synchronisation.
 * qt_metrics_finalize, one launch of one workgroup: state -> report, 4 C + 12 doubles (qt_metrics_report_bytes).  Counts
 * are added as integers, everything else is double arithmetic.  With support_i = sum_j cm[i][j], predicted_j = sum_i
 * cm[i][j], tp_k = cm[k][k], n = sum_i support_i:
 *   [0, C)      precision_k = tp_k / predicted_k        [C, 2C)   recall_k = tp_k / support_k
 *   [2C, 3C)    f1_k = 2 tp_k / (support_k + predicted_k)          [3C, 4C)  support_k
 *               (a zero denominator gives 0: scikit-learn's zero_division=0)
 *   4C + 0      accuracy = sum_k tp_k / n
 *   4C + 1..3   weighted precision / recall / F1: sum_k support_k x_k / n
 *   4C + 4..6   macro precision / recall / F1: the mean over the classes with support_k + predicted_k > 0 (scikit-learn's
 *               rule when no labels= is passed)
 *   4C + 7      R^2 of label index against predicted index (analysis.py:89): 1 - SS_res / SS_tot with
 *               SS_res = sum_ij cm[i][j] (i - j)^2, SS_tot = sum_i support_i (i - mean)^2, mean = sum_i i support_i / n;
 *               SS_tot == 0: 1.0 when SS_res == 0, else 0.0; n < 2: NaN
 *   4C + 8..11  n (samples), rows ignored, rows invalid, the number of classes with support_k + predicted_k > 0
 * With n == 0 accuracy and the six averages are NaN and the per-class values are 0.
 * QT_ERR_INVALID_ARG (before any device call) for a null desc, both or neither of logits / pred_in, probs / confidence /
 * pred_out without logits, labels without a state or a state without labels, a call that would produce nothing, ld < C,
 * ld_probs < C, rows <= 0, C <= 0, misaligned pointers (4 bytes for f32, 8 for the 64-bit arrays); QT_ERR_UNSUPPORTED for
 * C > 1024, rows > 2^22 and a dtype other than QT_F32. */
#define QT_METRICS_MAX_CLASSES 1024
typedef struct qt_metrics_desc {
  int dtype;                  /* of the logits: QT_F32 */
  long long ignore_index;     /* torch's default: -100 */
} qt_metrics_desc;
size_t qt_metrics_state_bytes(int C);
size_t qt_metrics_report_bytes(int C);
int qt_metrics_update(const qt_metrics_desc* desc, const float* logits, long long ld, const long long* pred_in,
                      const long long* labels, long long rows, int C, unsigned long long* state, float* probs,
                      long long ld_probs, float* confidence, long long* pred_out, void* stream);
int qt_metrics_finalize(const unsigned long long* state, int C, double* report, void* stream);
/* Score-based evaluation: what the confusion matrix cannot give because it needs the scores, not counts: top-k accuracy,
 * one-vs-rest ROC / AUC and average precision per class, and the calibration of the confidence (the value the caption shows
 * and PoseTimeline(min_confidence=) thresholds), without copying [rows][C] probabilities to the host every batch.  A second
 * meter in the image of qt_metrics_*: additive integer state in device memory, one launch per batch, one finalize, integers
 * wherever the result must not depend on order, so the same bits on every run.
 * Inputs.  scores f32 [rows][C], row stride ld >= C elements (padding columns are never read into a result), labels int64
 * [rows]; 1 <= C <= QT_SCORES_MAX_CLASSES, 1 <= rows <= 2^22 per call.  desc->kind:
 *   QT_SCORES_LOGITS   p is qt_metrics_update's softmax (m = z[argmax], e_k = expf(z_k - m), s = sum_k e_k, p_k = e_k / s,
 *                      same lane mapping and summation order): the bits qt_metrics_update writes to probs
 *   QT_SCORES_PROBS    p is the row as given (e.g. qt_timeline_smooth's smoothed rows)
 * Row classes, the first that applies:  ignored (label == desc->ignore_index), invalid (label outside [0, C)), nan (some
 * p_k is NaN, or, with QT_SCORES_PROBS, outside [0, 1]), counted.  Only counted rows reach the tables.
 * Score key.  K = 1 << desc->bits, QT_SCORES_MIN_BITS <= bits <= QT_SCORES_MAX_BITS;  q(p) = min(K - 1, (int)(p * (float)K)):
 * a multiplication by a power of two and a truncation, both exact in f32.
 * State, u64, zeroed once by the caller and only ever added to; qt_scores_state_bytes(C, bits, M) = 8 (2 C K + C + 3 M + 5):
 *   hist[C][2][K]   hist[(k * 2 + side) * K + q(p_k)] += 1 for every class k of a counted row; side = 1 when the label is k
 *   rank[C]         rank[r] += 1 with r = #{k : s_k > s_y, or s_k == s_y and k < y}, y the label, s the scores AS GIVEN (z for
 *                   logits, p for probs).  rank[0] is torch.max's hit count; top_k = sum_{r < k} rank[r] / counted
 *   cal[M][3]       1 <= M = desc->cal_bins <= QT_SCORES_MAX_CAL_BINS.  pred = argmax of p in the loss head's total order (the
 *                   larger value, then the lower index), conf = p[pred], bin = min(M - 1, (int)(conf * (float)M)) with the
 *                   product rounded to f32;  cal[bin] += { 1, pred == y, rint(clamp(conf, 0, 1) * 65536) }  (the integer
 *                   confidence of qt_timeline_decode, for the same reason: a sum that does not depend on order)
 *   counters[5]     rows counted, ignored, invalid, nan; update calls
 * Every add is an integer atomic: the states of several calls, streams, devices or ranks add up to the state of their
 * union, and a batch split into calls at any row gives the bits of one call (but for the update counter).
 * qt_scores_update, one launch, no workspace, no zero fill, no host synchronisation.  desc->route: QT_SCORES_ROUTE_DIRECT (one
 * 64-bit global atomic per cell of a counted row), QT_SCORES_ROUTE_PRIVATE (a workgroup owns QT_SCORES_SLICE_ROWS rows and one
 * class, counts in a u32 LDS histogram and adds its non-zero cells), QT_SCORES_ROUTE_AUTO (private from
 * QT_SCORES_AUTO_PRIVATE_ROWS rows on: a measurement, EXPERIMENTS.md "Score metrics").  The routes give the same state.
 * qt_scores_finalize: state -> report, 4 C + 3 M + 12 doubles (qt_scores_report_bytes(C, M)); counts are added as integers,
 * everything else is double arithmetic in a fixed order.  Per class k with pos_b = hist[k][1][b], neg_b = hist[k][0][b],
 * P = sum_b pos_b, N = sum_b neg_b, negbelow_b = sum_{b' < b} neg_b', tp_b = sum_{b' >= b} pos_b', fp_b likewise:
 *   [0, C)     auc_k = A2 / (2 P N), A2 = sum_b pos_b (2 negbelow_b + neg_b) in 64-bit integers (exact while 2 P N < 2^64),
 *              one double division; NaN when P == 0 or N == 0.  The Mann-Whitney statistic of the quantised scores with
 *              ties at half credit: sklearn.metrics.roc_auc_score(y == k, q / K)
 *   [C, 2C)    ap_k = sum over the bins with pos_b > 0 of (pos_b / P) (tp_b / (tp_b + fp_b)): a thread sums its K / 256
 *              consecutive bins from the top down (K < 256: one bin), the 256 partial sums are added by the halving tree
 *              red[t] += red[t + s], s = 128 .. 1; NaN when P == 0.  sklearn.metrics.average_precision_score(y == k, q / K)
 *   [2C, 3C)   support_k = P
 *   [3C, 4C)   top_k for k = 1 .. C (index k - 1): integer partial sums of rank over counted; NaN when nothing was counted
 *   4C + [0, M) rows of the bin, + [M, 2M) accuracy = hits / rows, + [2M, 3M) mean confidence = sum / (65536 rows); an empty
 *              bin gives 0
 *   then 12 scalars: macro AUC, support-weighted AUC (over the classes whose AUC is defined, ascending k), macro AP,
 *              support-weighted AP (likewise), ece = sum_b (n_b / n) |acc_b - conf_b| over the occupied bins in ascending
 *              order, mce = the largest such gap (both NaN when n == 0), samples, ignored, invalid, nan rows, classes scored
 *              (those with a defined AUC), update calls
 * curves (or NULL): int64 [C][2][K], curves[k][0][b] = tp_b, curves[k][1][b] = fp_b; dividing by P and N gives the ROC and
 * precision / recall points, no float curve is stored.
 * Both size queries return 0 for an argument outside its range.  QT_ERR_INVALID_ARG (before any launch; qt_last_error names
 * the entry point) for a null desc, kind / bits / cal_bins / route outside their ranges, null scores / labels / state /
 * report, rows <= 0, C <= 0, ld < C, misaligned pointers (4 bytes for f32, 8 for the 64-bit arrays); QT_ERR_UNSUPPORTED for
 * C > QT_SCORES_MAX_CLASSES, rows > 2^22 and a dtype other than QT_F32. */
#define QT_SCORES_MAX_CLASSES 64
#define QT_SCORES_MAX_CAL_BINS 64
#define QT_SCORES_MIN_BITS 4
#define QT_SCORES_MAX_BITS 14
#define QT_SCORES_SLICE_ROWS 1024
#define QT_SCORES_AUTO_PRIVATE_ROWS 64
enum { QT_SCORES_LOGITS = 0, QT_SCORES_PROBS = 1 };
enum { QT_SCORES_ROUTE_AUTO = 0, QT_SCORES_ROUTE_DIRECT = 1, QT_SCORES_ROUTE_PRIVATE = 2 };
typedef struct qt_scores_desc {
  int dtype;                  /* of the scores: QT_F32 */
  int kind;                   /* QT_SCORES_LOGITS | QT_SCORES_PROBS */
  int bits;                   /* K = 1 << bits score bins */
  int cal_bins;               /* M calibration bins */
  int route;                  /* QT_SCORES_ROUTE_* */
  long long ignore_index;     /* torch's default: -100 */
} qt_scores_desc;
size_t qt_scores_state_bytes(int C, int bits, int cal_bins);
size_t qt_scores_report_bytes(int C, int cal_bins);
int qt_scores_update(const qt_scores_desc* desc, const float* scores, long long ld, const long long* labels, long long rows,
                     int C, unsigned long long* state, void* stream);
int qt_scores_finalize(const unsigned long long* state, int C, int bits, int cal_bins, double* report, long long* curves,
                       void* stream);
/* Annotated frames: the last step of the reference's video loop (experiment/test_on_video_cnn.py:280-295: draw_landmarks,
 * putText, then the writer) and the drawing step of sqn process/processing_image_sequence.py:250-318 (draw_enhanced_skeleton),
 * resnet/grad_cam_analysis.py:437 and grad_cam/5_grad_cam_visualizer.py, for a whole batch of uint8 frames in one launch, from
 * tensors that are already on the device (the landmarks qt_pose_features takes, the pred / confidence qt_metrics_update
 * writes): no host read of a prediction, one copy of the finished frames.
 * frames, out: uint8 [batch][H][W][3], contiguous, any address; out == frames is allowed, no other overlap.  Two groups of
 * operands, each given whole or not at all, at least one of them:
 *   skeleton  landmarks f32 [batch][33][4] = x, y, z, visibility (16-byte aligned); segments uint8 [n_segments][3] = landmark
 *             a, landmark b, major flag, in DEVICE memory, 0 <= n_segments <= QT_ANNOTATE_MAX_SEGMENTS; detected uint8 [batch]
 *             or NULL (every frame detected).
 *   caption   pred int64 [batch]; atlas uint8 [num_classes + 14][glyph_h][glyph_w] coverage masks and atlas_widths int32
 *             [num_classes + 14]: glyph g < num_classes is the pre-rendered caption of class g (whatever string the caller
 *             rendered, e.g. "Pose: Tadasana"), then '0'..'9', '.', '(', ')', ' '; confidence f32 [batch] or NULL.
 * The rule per frame, every coordinate an exact integer:
 *   1. P_j = (trunc(x_j W), trunc(y_j H)): the product in f32, truncated toward zero (Python's int()).  Landmark j is usable
 *      when both products are finite and lie in [-8192, 16383]; a primitive that needs an unusable landmark is skipped, and so
 *      is a segment with a landmark index above 32 (nothing is indexed with it).  A frame with detected == 0 gets no skeleton.
 *   2. Segment (a, b, major): T = major ? thick_major : thick_minor; colour line_hi when both visibilities are
 *      > min_visibility, else line_lo (a NaN visibility is low).  Pixel q is covered iff 4 dist^2(q, segment) <= T^2, taken
 *      as: d = P_b - P_a, e = q - P_a, L = d.d, t = e.d;  L == 0 or t <= 0: 4 e.e <= T^2;  t >= L: 4 |q - P_b|^2 <= T^2;
 *      otherwise cross = e.x d.y - e.y d.x and cross^2 <= floor(T^2 L / 4).  (|cross| < 2^31 and every product fits a signed
 *      64-bit integer for H, W <= 8192, T <= 15 and usable landmarks.)
 *   3. Landmark j: the disc |q - P_j|^2 <= r^2 with r = radius_hi and point_hi when its visibility is > min_visibility, else
 *      radius_lo and point_lo.
 *   4. Painter's order: the segments in list order, then landmarks 0 .. 32; the last primitive that covers a pixel wins,
 *      drawing is opaque (draw_enhanced_skeleton's two passes).
 *   5. The caption, over the skeleton (putText follows draw_landmarks): none when pred[b] is outside [0, num_classes) (only
 *      the device sees it).  Otherwise the glyphs are pred[b], followed, when confidence is given and not NaN, by
 *      ' ' '(' d0 '.' d1 d2 ')' with n = clamp((int)rintf(confidence * 100.0f), 0, 100) and the digits n / 100, n / 10 % 10,
 *      n % 10.  Glyph k occupies columns [pen_k, pen_k + width_k) and rows [oy, oy + glyph_h); pen_0 = ox; a width outside
 *      [0, glyph_w] counts as 0.  Where its mask m > 0: out_c = (m colour_c + (255 - m) under_c + 127) / 255 in integers.
 *   6. Everything is clipped to the frame; every other pixel of out equals frames.
 * Colours are bytes in the frames' channel order.
 * Against the reference: it multiplies in float64, so a product within one f32 rounding of an integer can land in the
 * neighbouring pixel; f"{confidence:.2f}" can differ in the last digit where confidence * 100 rounds in f32 to within one
 * step of a half.  cv2.line draws thick lines as filled polygons with round caps in fixed point and cv2.circle its own
 * midpoint discs: bit equality with them is not claimed, the rule above is the exact Euclidean one.  MediaPipe's own default
 * drawing style (test_on_video_cnn.py) is not reproduced, the style is draw_enhanced_skeleton's.  Text is the caller's atlas,
 * not Hershey strokes.
 * One launch: a workgroup owns 4096 consecutive pixels of one frame, lists in LDS the primitives whose bounding box meets
 * them, and each thread owns 16 pixels = three 16-byte stores (16-byte loads where frames and out agree modulo 16, scalar
 * heads and tails per frame).  With out == frames, pixels no primitive can reach are neither read nor written.  No workspace,
 * no atomics, no zero fill, no host synchronisation; nothing outside the stated extents is read or written; the same bits on
 * every run and for a frame alone or inside a batch.
 * QT_ERR_INVALID_ARG (before any device call) for a null desc, non-positive batch / H / W, n_segments outside
 * [0, QT_ANNOTATE_MAX_SEGMENTS], a thickness or radius outside [1, 15] or a NaN min_visibility (the three with a skeleton;
 * a caption alone does not read them), null frames / out, out that overlaps frames without being equal to it, a group given in part (landmarks without segments or the reverse, detected
 * without landmarks; pred, atlas, atlas_widths not all three; confidence without them), neither group, misaligned
 * landmarks (16) / pred (8) / confidence and atlas_widths (4), and with a caption num_classes, glyph_h or glyph_w below 1;
 * QT_ERR_UNSUPPORTED for H or W above 8192, more than 2^31 bytes of frames, glyph_h or glyph_w above 8192, |ox| or |oy|
 * above 2^20. */
#define QT_ANNOTATE_MAX_SEGMENTS 64
typedef struct qt_annotate_desc {
  int batch, H, W, n_segments;
  float min_visibility;             /* 0.65 in the reference's call */
  int thick_major, thick_minor;     /* 5 and 2 */
  int radius_hi, radius_lo;         /* 3 and 2 */
  unsigned char line_hi[3], line_lo[3], point_hi[3], point_lo[3];
  int num_classes, glyph_h, glyph_w;
  int ox, oy;                       /* top-left of the first glyph */
  unsigned char caption_colour[3];
} qt_annotate_desc;
int qt_annotate_u8(const qt_annotate_desc* desc, const unsigned char* frames, const float* landmarks,
                   const unsigned char* detected, const unsigned char* segments, const long long* pred,
                   const float* confidence, const unsigned char* atlas, const int* atlas_widths, unsigned char* out,
                   void* stream);
/* Pose timeline: what lies between the per-frame probabilities of the video loop (qt_metrics_update's probs) and what a
 * practitioner is shown or told: a trailing-window mean of the probabilities with its argmax and confidence
 * (qt_timeline_smooth), then a debounced label per frame and the list of segments "which pose from when to when"
 * (qt_timeline_decode).  The reference has no such step (experiment/test_on_video_cnn.py:274-292 writes each frame's raw
 * argmax), so nothing of it is restated here.  batch = streams (videos, or the camera feeds of a live loop), frames = this
 * call's frames per stream: qt_pose_sequence_features' layout.  Both calls take the one descriptor and read their own fields.
 *
 * qt_timeline_smooth (reads batch, frames, num_classes = C, window = W).  probs: f32 [batch][frames][C], row stride ld >= C
 * elements, a stream's rows `frames * ld` apart; padding columns are neither read into a result nor written.  For frame f of a
 * stream, with seen = min(hist_count_in, W - 1) the rows its history holds (0 without a history):
 *   n = min(W, seen + f + 1)
 *   s_k = p[f-n+1][k]; then s_k = s_k + p[g][k] for g = f-n+2 .. f, one f32 add after the other, oldest row first, formed
 *         afresh for every frame (no running sum: it would drift, keep a NaN for ever, and depend on where a call starts);
 *   m_k = s_k / (float)n, the IEEE f32 quotient; a NaN m_k is stored as the quiet NaN 0x7fc00000 (sign and payload of a
 *         computed NaN differ between processors; a number is never touched)
 * where p[g] for g < 0 is hist_in slot -1 - g.  NaN and inf go by IEEE rules into the n frames that read them.
 *   pred        int64 [batch][frames]: argmax_k m_k by the loss head's total order (a NaN beats every number, then the larger
 *               value, then the lower index), the order of qt_loss_forward and qt_metrics_update
 *   confidence  f32 [batch][frames]: m[pred]
 *   smoothed    f32 [batch][frames][C], row stride ld_smoothed >= C, or NULL
 * pred and confidence are both required (they are what qt_annotate_u8 and qt_timeline_decode take).
 * History across calls.  hist_in: f32 [batch][W-1][C] dense, the last W - 1 rows before this call, slot 0 the most recent;
 * hist_count_in: int32 [batch], how many slots hold a row (a value above W - 1 counts as W - 1, a negative one as 0; a zeroed
 * count is an empty stream); slots at and beyond the count are not read.  hist_out / hist_count_out: the same state after the
 * call's last frame, rows copied bit for bit, slots beyond the count written as zeros.  Both pairs NULL: every stream starts
 * empty and nothing is kept.  With W == 1 there is no history: the pointers are not looked at.  hist_out must not overlap
 * hist_in, nor hist_count_out hist_count_in (other workgroups still read them): a caller swaps two buffers.  A stream
 * processed in any split into consecutive calls gives the same bits as one call: a predecessor row is the same value from
 * probs or from the history and goes through the same additions in the same order.
 * One launch: a workgroup owns QT_TIMELINE_TILE consecutive frames of one stream, stages them and the W - 1 rows in front of
 * them in LDS (16-byte loads where ld, C and the addresses are multiples of four floats, single floats otherwise), sums with
 * thread = (frame, class) and takes the argmax across the class lanes (one 16-lane DPP row for C <= 16, a wave above); the
 * workgroup that owns a stream's last frame writes the history.  No atomics, no zero fill, no workspace, no host
 * synchronisation; the same bits on every run and for a stream alone or in a batch; inputs are never written; nothing
 * outside [0, frames) of a stream and the history's counted slots is read.
 *
 * qt_timeline_decode (reads batch, frames, num_classes, min_run, min_confidence, capacity, flush).  pred: int64
 * [batch][frames], confidence: f32 [batch][frames]; state: int64 [batch][QT_TIMELINE_STATE], in device memory for the whole
 * video, updated in place:
 *   { frames_seen, stable + 1, cand + 1, run, seg_start, seg_len, seg_conf_sum, segments_total }
 * Labels are stored plus one, so a zeroed state is the initial state (the caller zeroes it once).  Per stream, frame by frame
 * in order, t = frames_seen + f:
 *   c = (confidence >= min_confidence && 0 <= pred < C) ? pred : -1          (a NaN confidence gives -1)
 *   c == cand: run = min(run + 1, 2^31 - 1); otherwise cand = c, run = 1
 *   run >= min_run: stable = cand      (so min_run unknown frames in a row make the label unknown again)
 *   stable[f] = stable, int64 [batch][frames], -1 for none (qt_annotate_u8 draws no caption for it)
 * A segment is a maximal run of frames with one stable >= 0; a run of -1 is a gap, not a segment.  When stable changes at
 * frame t, the open segment (if seg_len > 0) is closed, and a stable >= 0 opens one with seg_start = t.  Every frame of an
 * open segment adds 1 to seg_len and q(confidence) to seg_conf_sum, q(x) = (long long)rintf(min(max(x, 0), 1) * 65536.0f)
 * and q(NaN) = 0: integer sums, so the mean confidence seg_conf_sum / (65536 seg_len) is the same whatever the split into
 * calls.  Closing writes { start, length, label, conf_sum } to segments[b][segments_total] (int64 [batch][capacity][4]) if
 * segments_total < capacity, and adds 1 to segments_total either way; records at and behind it are not written.  Slots are
 * cumulative across calls: the buffer is the video's list, ascending by start.  With no segment open seg_start, seg_len and
 * seg_conf_sum are 0.  flush != 0 also closes the segment that is open after the call's last frame (end of the video) and
 * leaves seg_start = frames_seen, seg_len = seg_conf_sum = 0; the label stays, and a later frame with the same stable label
 * opens a new segment at its own number.  frames == 0 with flush is allowed (pred, confidence, stable are not looked at).
 * One launch: one workgroup (one wave) per stream walks its frames in trips of QT_TIMELINE_TRIP, lane = frame; inside a trip
 * the run length, the stable label and the segment bounds are "last qualifying lane" scans over ballots, the confidence sums
 * an integer prefix sum (DPP shifts), the slots a ballot rank on segments_total; the carry between trips is read from the
 * trip's last lane into scalars.  No workgroup waits
 * for another, no atomics, no zero fill, no workspace, no host synchronisation; the same bits on every run, for any split
 * into calls and for a stream alone or in a batch.
 *
 * QT_ERR_INVALID_ARG (before any device call, qt_last_error names the argument) for a null desc, non-positive batch,
 * negative frames or zero frames (decode: without flush), num_classes outside 1 .. QT_TIMELINE_MAX_CLASSES, smooth: window
 * outside 1 .. QT_TIMELINE_MAX_WINDOW, ld < C, ld_smoothed < C, half a history pair, histories that overlap, smoothed that
 * overlaps probs; decode: min_run < 1, a NaN min_confidence, a negative capacity, segments == NULL with capacity > 0; null or
 * misaligned pointers (4 bytes for f32 and int32, 8 for int64); QT_ERR_UNSUPPORTED for more than 2^22 frames in all. */
#define QT_TIMELINE_MAX_CLASSES 64
#define QT_TIMELINE_MAX_WINDOW 64
#define QT_TIMELINE_TILE 64
#define QT_TIMELINE_TRIP 64
#define QT_TIMELINE_STATE 8
typedef struct qt_timeline_desc {
  int batch;                        /* streams */
  int frames;                       /* frames per stream in this call */
  int num_classes;                  /* C, 1 .. 64 */
  int window;                       /* W, 1 .. 64: smooth */
  int min_run;                      /* >= 1: decode */
  float min_confidence;             /* not NaN: decode */
  int capacity;                     /* records per stream in `segments`: decode */
  int flush;                        /* != 0: close the open segment after the last frame: decode */
} qt_timeline_desc;
int qt_timeline_smooth(const qt_timeline_desc* desc, const float* probs, long long ld, const float* hist_in,
                       const int* hist_count_in, float* hist_out, int* hist_count_out, float* smoothed, long long ld_smoothed,
                       long long* pred, float* confidence, void* stream);
int qt_timeline_decode(const qt_timeline_desc* desc, const long long* pred, const float* confidence, long long* state,
                       long long* stable, long long* segments, void* stream);
/* Segment-level evaluation: the segmental edit score and the segmental F1 at IoU thresholds (Lea et al., CVPR 2017; the MS-TCN
 * evaluation: Edit, F1@10/25/50) of a per-frame labelling against the ground truth, counted in integers on the device and added
 * to a state in device memory.  qt_metrics_update and qt_scores_update count frames: a prediction that splits every pose hold
 * into five fragments scores there almost as a clean one.  These counts see runs: what qt_timeline_decode's stable labels,
 * qt_pose_order_decode's path classes and a raw argmax differ in.  The reference has no such step (comparative analysis/
 * analysis.py:60-109 counts frames), so nothing of it is restated here.
 *
 * Inputs.  Per call `batch` WHOLE videos.  pred, label: int64 [batch][frames], row strides ld_pred, ld_label >= frames
 * elements; padding columns are never read.  lengths: int32 [batch] or NULL: video b has len_b = clamp(lengths[b], 0, frames)
 * frames, NULL means frames; frames at and beyond len_b are never read.
 * Runs.  A frame's value v is KNOWN when 0 <= v < C.  A run is a maximal stretch of consecutive frames of one video that hold
 * the same known value; unknown frames belong to no run and are a gap, as in qt_timeline_decode, so two runs of one class with
 * a gap between them are two runs.  A run is { start, length, class }.  P = the runs of pred (m of them), Y = the runs of label
 * (n of them), both in order of start.
 * Per video, all in integers:
 *   frames_labelled  frames whose label is known;  frames_correct  those of them with pred == label
 *   overflow         m > QT_SEGMENTS_MAX or n > QT_SEGMENTS_MAX: the record holds the true m and n, D = -1 and every tp_k = -1;
 *                    the frame counts still count; the video adds to videos_overflow and to nothing else below
 *   D                the Levenshtein distance of the class sequences of P and Y, insertion, deletion and substitution 1 each:
 *                    D[i][j] = min(D[i-1][j] + 1, D[i][j-1] + 1, D[i-1][j-1] + (p_i != y_j)), D[i][0] = i, D[0][j] = j
 *   edit_q           with M = max(m, n) > 0: ((M - D) * 2^32) / M, a division of int64; M == 0: the video is EMPTY and adds
 *                    nothing to the edit sums
 *   partner          of a predicted run p among the true runs y of p's class, end = start + length:
 *                      inter = max(0, min(p_end, y_end) - max(p_start, y_start)),  union = max(p_end, y_end) - min(p_start, y_start)
 *                    the y with the largest inter / union, fractions compared by cross-multiplication in int64, ties to the lowest
 *                    index; none when Y has no run of that class
 *   tp_k             p PASSES threshold k (pct_k in 1 .. 100, 1 <= K <= 8) when it has a partner and 100 inter >= pct_k union;
 *                    tp_k = the number of DISTINCT true runs that are the partner of at least one passing predicted run;
 *                    fp_k = m - tp_k, fn_k = n - tp_k
 * (In the published loop each predicted run in turn claims its best partner and is a false positive if that one is taken.  For
 * thresholds above zero both forms count the same: tests/_segments_ref.py holds both.)
 *   records  int64 [batch][QT_SEGMENTS_RECORD + K] or NULL:  { m, n, D, frames_labelled, frames_correct, tp_0 .. tp_{K-1} }
 *   state    int64 [QT_SEGMENTS_STATE + K], zeroed once by the caller, added to by every call:
 *            { videos, videos_overflow, videos_empty, seg_pred, seg_true, edit_dist, edit_max, edit_q, frames_labelled,
 *              frames_correct, tp_0 .. }
 *            seg_pred = sum m, seg_true = sum n, edit_dist = sum D, edit_max = sum M, edit_q and tp_k over the videos that do
 *            not overflow; the frame counts over all.  The state is additive: any split of the videos into calls, any order and
 *            a sum of per-rank states give the same bits.
 * The report is the caller's arithmetic on one copy of the state (no kernel), a zero denominator giving 0:
 *   edit = 100 edit_q / (2^32 (videos - videos_overflow - videos_empty)),  edit_micro = 100 (1 - edit_dist / edit_max)
 *   precision_k = 100 tp_k / seg_pred,  recall_k = 100 tp_k / seg_true,  f1_k = 100 * 2 tp_k / (seg_pred + seg_true)
 *   frame_accuracy = frames_correct / frames_labelled,  over_segmentation = seg_pred / seg_true
 * workspace: qt_segments_workspace_bytes(desc) bytes (batch records), 8-byte aligned, always required.
 * Two launches.  One workgroup of 256 threads per video: (a) frames in trips of 256, thread = frame; the thread at a run's last
 * frame writes the run, its slot the ballot rank (64-bit ballots) of its end plus the ends of the waves and trips before, its
 * start the last start flag at or before it; runs go to LDS up to QT_SEGMENTS_MAX, m and n go on counting; (b) the frame
 * counts; (c) the Levenshtein table by anti-diagonals, three rotating diagonals of QT_SEGMENTS_MAX + 1 int32 in LDS, one
 * barrier per diagonal; (d) thread = predicted run, a plain scan of the true runs, an LDS flag per (partner, threshold),
 * counted by ballot; (e) the record goes to the workspace.  Then ONE workgroup adds the records of the workspace to the state
 * (integer atomics) and copies them to `records`.  40 KiB of static LDS.  No workgroup waits for another inside a launch, no
 * zero fill, no host synchronisation; inputs are never written; nothing outside [0, len_b) of a row is read.
 *
 * qt_segments_encode (reads batch, frames, num_classes, capacity) is the run extraction alone, the same device function: the
 * first `capacity` runs of values (int64 [batch][frames], row stride ld) go to runs: int32 [batch][capacity][3] = { start,
 * length, class }, the true number of runs to counts: int32 [batch], as qt_timeline_decode does with segments_total; records
 * at and behind the count are not written.  One launch, one workgroup per video.
 *
 * QT_ERR_INVALID_ARG (before any device call, qt_last_error names the argument) for a null desc, batch < 1, frames < 0,
 * num_classes outside 1 .. QT_SEGMENTS_MAX_CLASSES, update: num_thresholds outside 1 .. QT_SEGMENTS_MAX_THRESHOLDS, a pct outside
 * 1 .. 100, ld_pred or ld_label < frames, a null state or workspace, a workspace that is too small; encode: ld < frames, a
 * negative capacity, runs == NULL with capacity > 0, null counts; null (with frames > 0) or misaligned pointers (8 bytes for
 * int64, 4 for int32).  QT_ERR_UNSUPPORTED for more than 2^22 frames (or videos) in all.  frames == 0 is allowed: every video
 * is then empty, and pred, label and values are not looked at. */
#define QT_SEGMENTS_MAX 1024
#define QT_SEGMENTS_MAX_CLASSES 1024
#define QT_SEGMENTS_MAX_THRESHOLDS 8
#define QT_SEGMENTS_RECORD 5
#define QT_SEGMENTS_STATE 10
typedef struct qt_segments_desc {
  int batch;                        /* videos in this call */
  int frames;                       /* columns per video; a video's own length is lengths[b] */
  int num_classes;                  /* C, 1 .. 1024 */
  int num_thresholds;               /* K, 1 .. 8: update */
  int pct[8];                       /* IoU thresholds in per cent, 1 .. 100, the first K are read: update */
  int capacity;                     /* runs per video in `runs`: encode */
} qt_segments_desc;
size_t qt_segments_workspace_bytes(const qt_segments_desc* desc);
int qt_segments_update(const qt_segments_desc* desc, const long long* pred, long long ld_pred, const long long* label,
                       long long ld_label, const int* lengths, long long* state, long long* records, void* workspace,
                       size_t workspace_bytes, void* stream);
int qt_segments_encode(const qt_segments_desc* desc, const long long* values, long long ld, const int* lengths, int* runs,
                       int* counts, void* stream);
/* Pose-order decoding: the best path of a hidden-Markov chain whose STATES are the steps of the pose sequence (the twelve
 * steps of a Sun Salutation, in their cyclic order), each state emitting one of the C classes, over the probabilities of the
 * video loop (qt_metrics_update's probs, or qt_timeline_smooth's smoothed rows).  The debounced argmax of qt_timeline_decode
 * treats the classes as unrelated labels; this decode knows their order, tells the two occurrences of a pose inside one round
 * apart, and its path is what rounds are counted on.  The reference has no such step.  Every number is an integer from the
 * emission score on, so every output is the same bits on every run and for any split of a stream into calls.
 *
 * probs: f32 [batch][frames][C], row stride ld >= C, a stream's rows `frames * ld` apart; state_class: int32 [S], the class
 * a state emits; trans: int32 [S][S], trans[i][j] the score of going from state i to state j between two frames, in
 * [-65536, 0]; init: int32 [S] in the same range, the scores before a stream's first frame, or NULL for zeros.  state_class,
 * trans and init are in device memory: an entry of trans or init outside the range is clamped into it as it is read, and a
 * state whose class is outside [0, C) scores the floor -8192 at every frame and indexes nothing.  carry: int64
 * [batch][S + 2] = { frames_seen, score_offset, delta[S] }, in device memory for the whole video, updated in place; the caller
 * zeroes it once.
 * Emission score q(p) of an f32 p with bit pattern b, in units of 1/256 bit:
 *   p is NaN or p < 2^-32 (negatives, zeros, denormals): q = -8192
 *   p >= 1 (+inf too):                                    q = 0
 *   otherwise:  q = 256 ((b >> 23) - 127) + LOG2_TABLE[(b >> 15) & 255],  LOG2_TABLE[i] = rint(256 log2(1 + (2 i + 1) / 512))
 * (1, 2, 4, 5 ... 254, 255, 256; no entry is closer than 0.0015 to a half; the table is written out in csrc/pose_chain.h).
 * q stays within 1.25 units of 256 log2 p, and no logf enters the rule.  e[f][s] = q(probs[f][state_class[s]]).
 * Forward, per stream, frame by frame; d is the previous frame's scores: init for the stream's first frame (frames_seen ==
 * 0), carry.delta otherwise:
 *   psi[f][j]   = the LOWEST i that attains max_i (d[i] + trans[i][j])
 *   delta[f][j] = that maximum + e[f][j]
 *   filtered[f] = the lowest j that attains max_j delta[f][j]        (causal: usable frame by frame in a live loop)
 * Backtrace, per call:  path[frames - 1] = filtered[frames - 1],  path[f - 1] = psi[f][path[f]].
 * Carry out:  frames_seen += frames;  m = max_j delta[last][j];  carry.delta = delta[last] - m;  score_offset += m.
 *   path        int64 [batch][frames], required
 *   filtered    int64 [batch][frames], or NULL
 *   emissions   int32 [batch][frames][S], or NULL
 * Split contract.  Subtracting a constant changes no argmax, so for a stream handed over in any split into consecutive calls
 * filtered, emissions and the final carry are the bits of one call, and the LAST call's path is the one-call path on its
 * frames; the paths of earlier calls are the best paths given what had been seen by then and are not revised.
 * Routes.  frames <= QT_POSE_ORDER_TILE: one launch, one wave per stream, lane = state, the tile's emissions, the table and
 * psi in LDS, no workspace (the live loop's route).  Longer calls: with M_f[i][j] = trans[i][j] + e[f][j] a frame is
 * delta_f = delta_(f-1) (x) M_f in the (max, +) semiring, and integer (max, +) products are exactly associative: (a) a
 * workgroup per tile forms the tile's product, (b) the start vector is carried through the products in order, on two levels
 * above 32 tiles (the tile products of a group of 32 multiplied into one, the stream's start carried through the group
 * products, then every group's start through its own tile products), (c) every tile replays its frames from its start
 * vector with the vector step, where psi and filtered get the rule's lowest-index ties, and composes its psi into one
 * back-map, (d) the tiles' end states follow from the last tile's by the back-maps, and every tile backtraces its own
 * frames.  Five launches (seven above 32 tiles), intermediate scores int32 inside a tile and int64 across tiles; only the
 * outputs are the contract.  qt_pose_order_workspace_bytes: what the tiled route needs (8-byte
 * aligned; every slot that is read is written in the same call, nothing is zero-filled), 0 on the short route and for a
 * descriptor that would be refused.  No workgroup waits for another inside a launch, no atomics, no host synchronisation;
 * inputs are never written; a stream alone gives the bits of the same stream in a batch.
 *
 * QT_ERR_INVALID_ARG (before any device call, qt_last_error names the argument) for a null desc, non-positive batch or
 * frames, num_states or num_classes outside 1 .. 64, ld < C, a null probs, state_class, trans, carry or path, misaligned
 * pointers (4 bytes for f32 and int32, 8 for int64 and the workspace), a workspace smaller than the query's size, an output
 * (carry, path, filtered, emissions, workspace) that overlaps an input or another output; QT_ERR_UNSUPPORTED for more than
 * 2^20 frames in all (batch * frames). */
#define QT_POSE_ORDER_TILE 64
#define QT_POSE_ORDER_MAX_STATES 64
#define QT_POSE_ORDER_MAX_CLASSES 64
typedef struct qt_pose_order_desc {
  int batch;                        /* streams */
  int frames;                       /* frames per stream in this call */
  int num_classes;                  /* C, 1 .. 64 */
  int num_states;                   /* S, 1 .. 64 */
} qt_pose_order_desc;
long long qt_pose_order_workspace_bytes(const qt_pose_order_desc* desc);
int qt_pose_order_decode(const qt_pose_order_desc* desc, const float* probs, long long ld, const int* state_class,
                         const int* trans, const int* init, long long* carry, long long* path, long long* filtered,
                         int* emissions, void* workspace, long long workspace_bytes, void* stream);
/* Pose-order posteriors: the marginals of the hidden-Markov chain that qt_pose_order_decode maximises: how sure the chain is
 * of step j at frame f.  Same inputs, limits and refusals: probs f32 [batch][frames][C] with row stride ld >= C, state_class
 * int32 [S], trans int32 [S][S] in [-65536, 0] (clamped as read), init int32 [S] or NULL for zeros, S and C <= 64, batch *
 * frames <= 2^20.  Emissions are the decoder's integers e[f][j] = q(probs[f][state_class[j]]), the same q bit for bit (NaN
 * and everything below 2^-32 give -8192, and so does a state whose class is outside [0, C)).
 * Scores are in units of 1/256 bit: T[i][j] = trans[i][j] / 256 and E[f][j] = e[f][j] / 256 are exact in f32, a path weighs
 * 2^(the sum of its T and E), the quantity the decoder maximises.  Write L_i x[i] = log2 sum_i 2^x[i].
 * Forward, per stream, frame by frame; a_prev is init / 256 at a stream's first frame (frames_seen == 0), the carry after it:
 *   A_f[j] = E[f][j] + L_i (a_prev[i] + T[i][j]),   c_f = L_j A_f[j],   a_f = A_f - c_f
 *   filtered[f][j] = 2^a_f[j]                        (causal; a row sums to 1)
 * Backward, over the call's n frames:  b_(n-1) = 0,  b_f[i] = L_j (T[i][j] + E[f+1][j] + b_(f+1)[j]), each frame's b less
 * its maximum (a constant changes no posterior; without it b falls by up to 288 a frame).
 *   posterior[f][j]       = 2^(a_f[j] + b_f[j] - L_k (a_f[k] + b_f[k]))     P(step j at frame f | every frame up to the call's end)
 *   class_posterior[f][c] = the sum of posterior[f][j] over the j with state_class[j] == c, in ascending j (0 where there is none)
 *   log2_evidence[stream] = sum_f c_f over the call, in bits, double
 * Every L is taken with its maximum out, L x = m + log2 sum_i 2^(x[i] - m) with m = max_i x[i], the sum in ascending i: it is
 * in [1, S], so no infinity or NaN arises for any table in range (an all -65536 table too: that is why the rule is in log2
 * and not in scaled probabilities, 2^-256 is no f32); a term more than 126 bits below the maximum may flush to zero.  c_f and
 * the evidence are accumulated in double.  carry: double [batch][S + 2] = { frames_seen, evidence_total, a_last[S] } in device
 * memory for the whole video, updated in place; the caller zeroes it once.  a_last holds f32 values, so the next call resumes
 * from the very a_f the last one ended on.
 *   posterior        f32 [batch][frames][S], required      filtered       f32 [batch][frames][S], or NULL
 *   class_posterior  f32 [batch][frames][C], or NULL       log2_evidence  double [batch], or NULL
 * Routes.  frames <= QT_POSE_ORDER_TILE: one launch, one wave per stream, lane = state, the emissions, the table and the a_f
 * rows in LDS, forward and then the backward sweep over the same rows, no workspace; at frames == 1 posterior == filtered.
 * Here filtered, evidence_total and the carry are the bits of one call for any split of a stream into such calls, and the last
 * call's posterior is the bits of the one-call posterior on its frames.  Longer calls: with M_f[i][j] = T[i][j] + E[f][j] a
 * frame is a_f = a_(f-1) (x) M_f in the (L, +) semiring and b_f = M_(f+1) (x) b_(f+1), so one set of tile products serves both
 * directions: (a) a workgroup per tile forms the tile's product, kept row-normalised (row maximum 0, the shifts summed per row
 * in double), (b) one wave per stream carries the start vector forward and the end vector backward through the products and
 * leaves every tile's start a, end b and the evidence before it, (c) a wave per tile replays its frames forward from its
 * start and sweeps backward from its end.  Three launches.  f32 (L, +) products are not exactly associative: this route's
 * outputs differ from the frame-by-frame rule by rounding, and the split promise in bits holds on the short route only.
 * qt_pose_posterior_workspace_bytes: what the tiled route needs (8-byte aligned; every slot that is read is written in the
 * same call, nothing is zero-filled), 0 on the short route and for a descriptor that would be refused.  No workgroup waits for
 * another inside a launch, no atomics, no host synchronisation; inputs are never written; a stream alone gives the bits of the
 * same stream in a batch; every run gives the same bits.
 *
 * QT_ERR_INVALID_ARG (before any device call, qt_last_error names the argument) for a null desc, non-positive batch or
 * frames, num_states or num_classes outside 1 .. 64, ld < C, a null probs, state_class, trans, carry or posterior, misaligned
 * pointers (4 bytes for f32 and int32, 8 for double and the workspace), a workspace smaller than the query's size, an output
 * (carry, posterior, filtered, class_posterior, log2_evidence, workspace) that overlaps an input or another output;
 * QT_ERR_UNSUPPORTED for more than 2^20 frames in all (batch * frames). */
long long qt_pose_posterior_workspace_bytes(const qt_pose_order_desc* desc);
int qt_pose_posterior(const qt_pose_order_desc* desc, const float* probs, long long ld, const int* state_class,
                      const int* trans, const int* init, double* carry, float* posterior, float* filtered,
                      float* class_posterior, double* log2_evidence, void* workspace, long long workspace_bytes, void* stream);
/* Pose-order prior learned on the device (Baum-Welch): the expected transition counts of the chain above under its own
 * posterior (qt_pose_prior_expect), the hard counts of given state paths (qt_pose_prior_count_paths), and the new tables from
 * the counts (qt_pose_prior_update).  Inputs, limits and notation are qt_pose_posterior's: E[f][j] = q(probs[f][state_class[j]])
 * / 256, T[i][j] = clamp(trans[i][j]) / 256, start[i] = clamp(init[i]) / 256 or 0 without init, L x = log2 sum 2^x with its
 * maximum out and its sum in ascending order.  Every sequence of a call is a WHOLE video: it starts from `start`, no carry is
 * read or written.
 * E-step, per sequence of n frames, with a_f and b_f the rows of the posterior rule (a_(-1) = start), for f = 0 .. n - 1:
 *   g_f[j]     = E[f][j] + b_f[j]
 *   x_f[i][j]  = a_(f-1)[i] + T[i][j] + g_f[j]
 *   Z_f        = L_(i,j) x_f[i][j]                   (the maximum out, i ascending, inside it j ascending)
 *   xi_f[i][j] = 2^(x_f[i][j] - Z_f)                 P(step i at frame f - 1 and step j at frame f | the whole video)
 *   counts[i][j]    += sum over f = 1 .. n - 1 of xi_f[i][j]
 *   start_counts[i] += sum over j of xi_0[i][j]      (frame 0's transition is the virtual one out of `start`: not in counts)
 *   totals[0]       += the sequence's evidence in bits (the posterior rule's log2_evidence);   totals[1] += n
 * Consequences: Z_f = L_i (a_(f-1)[i] + B_f[i]) with B_f[i] = L_j (T[i][j] + g_f[j]) the un-normalised b_(f-1), which is how
 * the kernel forms it; sum_j xi_f[i][j] is the posterior of frame f - 1 at i, sum_i xi_f[i][j] that of frame f at j; a
 * constant added to a_(f-1) or to b_f changes no xi.
 * counts double [S][S], start_counts double [S], totals double [2], in device memory, are ADDED TO (the caller zeroes them
 * once per E-step): a training set is one call per video, or one call per batch of videos of equal length.  The order of every
 * addition is fixed: the frames of a tile of QT_POSE_ORDER_TILE frames go, in the backward sweep's order (descending f), into an
 * f32 partial per (sequence, tile); a sequence's tiles are added in ascending order, then the sequences in ascending order,
 * both in double from zero, one thread per entry, and that sum is added onto the accumulator.  No float atomics, no zero
 * fill of caller memory, the same inputs give the same bits on every run.  frames == 1 adds zeros to counts.
 * Routes: frames <= QT_POSE_ORDER_TILE: a wave per sequence, then the reduction (two launches); longer calls: the posterior's
 * tile products and scan as they are, a replay per (sequence, tile) that stores no posterior rows, the reduction (four
 * launches), and as there the result differs from the frame-by-frame rule by f32 rounding.
 * Path counts, for path int64 [batch][frames] (a decoder's path for Viterbi training, or labelled steps):
 *   counts[p[f-1]][p[f]] += 1 for f >= 1;   start_counts[p[0]] += 1;   totals[1] += frames   (totals[0] is left alone)
 * A transition with an end outside [0, S) is left out, and so is a start outside it.  Per-workgroup integer histograms in
 * LDS, added in int64: exact integers in double.  num_classes of the descriptor is not used here.
 * M-step (one launch).  allowed int32 [S][S], non-zero where the transition may be learned (the learner fixes it when it is
 * made: the entry of the initial table is above -65536).  For row i, in double:
 *   r[j] = allowed[i][j] ? counts[i][j] + pseudo_count : 0;   R = sum_j r[j], ascending
 *   R > 0:   trans_out[i][j] = r[j] > 0 ? clamp(rint(256 log2(r[j] / R)), -65536, 0) : -65536
 *   otherwise the row keeps trans_in's values.
 * init_out, where not NULL, follows the same rule from start_counts with every entry allowed (old values init_in's, zeros
 * without one).  trans_out may be trans_in itself and init_out init_in itself.
 * qt_pose_prior_workspace_bytes: what qt_pose_prior_expect needs (never 0 for a descriptor in range: the partials; 8-byte
 * aligned; every slot that is read is written in the same call); it serves qt_pose_prior_count_paths too.  0 for a null or
 * out-of-range descriptor.
 *
 * QT_ERR_INVALID_ARG (before any device call, qt_last_error names the argument): as qt_pose_posterior for the descriptor, ld,
 * null and misaligned pointers (8 bytes for double, int64 and the workspace), the workspace's size and overlaps of an output
 * (counts, start_counts, totals, workspace; trans_out, init_out) with an input or another output; qt_pose_prior_update for
 * num_states outside 1 .. 64, a pseudo_count that is negative, NaN or infinite, a null counts, allowed, trans_in or trans_out,
 * an init_out without start_counts.  QT_ERR_UNSUPPORTED for more than 2^20 frames in all. */
long long qt_pose_prior_workspace_bytes(const qt_pose_order_desc* desc);
int qt_pose_prior_expect(const qt_pose_order_desc* desc, const float* probs, long long ld, const int* state_class,
                         const int* trans, const int* init, double* counts, double* start_counts, double* totals,
                         void* workspace, long long workspace_bytes, void* stream);
int qt_pose_prior_count_paths(const qt_pose_order_desc* desc, const long long* path, double* counts, double* start_counts,
                              double* totals, void* workspace, long long workspace_bytes, void* stream);
int qt_pose_prior_update(int num_states, const double* counts, const double* start_counts, const int* allowed,
                         double pseudo_count, const int* trans_in, const int* init_in, int* trans_out, int* init_out,
                         void* stream);
/* Fixed-lag pose-order posteriors and revised paths, for a loop that hands over a few frames (often one) per call: the answer
 * for the frame `lag` frames ago given everything up to now, a fixed delay behind the camera at a cost per step that does not
 * grow with the video.  The reference has no such step.  Tables, emissions q, T, E, L, clamping, the limits (S, C <= 64, batch
 * * frames <= 2^20) are qt_pose_posterior's and qt_pose_order_decode's; new is lag, 0 .. QT_POSE_LAG_MAX = 63, so that lag + 1
 * <= QT_POSE_ORDER_TILE and every window is a call of the short route.
 * Frames carry global indices g from the stream's start.  A call covers frames [seen, seen + n), n = desc->frames, its last
 * frame is last = seen + n - 1, and it EMITS frames [g0, g1):
 *   g0 = max(0, seen - lag),   g1 = flush ? seen + n : max(0, seen + n - lag),   count = g1 - g0
 * count is known to the host and may be 0 while the stream warms up; frames == 0 is allowed with flush only.  Output arrays are
 * [batch][count][...].  seen is host-known: all streams of a batch advance together.
 * qt_pose_lag_smooth.  Forward a_g, c_g, filtered, evidence_total: qt_pose_posterior's forward rule, frame by frame, the same
 * arithmetic in the same order (a_prev of frame 0 is init / 256 or zeros).  For each emitted g, with window end w = min(g +
 * lag, last):  b_w = 0,  b_f[i] = L_j (T[i][j] + E[f+1][j] + b_(f+1)[j]) less its maximum for f = w - 1 .. g,
 *   lagged[g][j]       = 2^(a_g[j] + b_g[j] - L_k (a_g[k] + b_g[k]));  where w == g the filtered row itself, bit for bit
 *   lagged_class[g][c] = the sum of lagged[g][j] over the j with state_class[j] == c, in ascending j
 *   lagged        f32 [batch][count][S], required when count > 0      lagged_class   f32 [batch][count][C], or NULL
 *   filtered      f32 [batch][n][S] (the new frames), or NULL         log2_evidence  double [batch] (this call's c_f), or NULL
 * qt_pose_lag_decode.  Forward delta, psi, filtered: the decoder's integer rule.  For each emitted g, with w as above:
 *   s = filtered[w];  s = psi[f][s] for f = w .. g + 1;  lag_path[g] = s
 *   lag_path      int64 [batch][count], required when count > 0       filtered       int64 [batch][n], or NULL
 * Carry.  Caller-owned device memory handed over as two buffers that must not overlap, carry_in (read; not read and may be NULL
 * with seen == 0) and carry_out (written in full); the caller swaps them between calls.  Per stream, smooth: { double
 * evidence_total, f32 a_last[S], f32 a[lag][S], int16 q[lag][S] }, decode: { int64 score_offset, int32 delta[S] (maximum 0),
 * uint8 psi[lag][S] }, each rounded up to 8 bytes; slot k of the history is frame seen + n - lag + k (zeros in front of the
 * stream's start).  qt_pose_lag_smooth_carry_bytes / qt_pose_lag_decode_carry_bytes give the size of one buffer.  lag, the
 * tables and batch are fixed for the life of a stream.
 * Contract.  For any split of a stream into calls, flush on the last, every output and the final carry are the bits of one
 * call, for both functions: the forward pass is the frame-by-frame rule on every route, and a window's arithmetic depends
 * neither on where a call boundary falls nor on the route.  Hence: lag == 0 gives filtered; with flush on the last call the
 * last lag + 1 frames carry the full posterior / path of a call ending there; a one-call flush with n <= lag + 1 is
 * qt_pose_posterior / qt_pose_order_decode on those frames (from zeroed carries).
 * Routes, the same bits on both.  Live: one launch, one wave per stream: table, carried history and new emissions in LDS, the
 * forward pass over the new frames, the count windows one after another, carry_out; no workspace.  Batch (catching up, a
 * recording): the same forward pass leaves its rows in the workspace (smooth: a and q; decode: psi and filtered), a second
 * launch runs the windows in parallel (smooth: a wave per emitted frame in groups of 16, decode: a thread per emitted frame).
 * One new frame goes live, and so do n frames (a flush alone: its pending frames) with n (lag + 1) <= 16 for smooth, <= 4096
 * for decode, whose walks are cheap; QTCNN_POSE_LAG=1 / 2 forces the live / the batch route (consulted per call, by the
 * workspace queries too).  qt_pose_lag_*_workspace_bytes: what the call needs (8-byte aligned, every slot that is read is written in the
 * same call), 0 on the live route and for a descriptor that would be refused.  No atomics, no zero fill of caller memory, no
 * host synchronisation, no workgroup waits for another inside a launch, inputs are never written, a stream alone gives the
 * bits it has in a batch.
 *
 * QT_ERR_INVALID_ARG (before any device call, qt_last_error names the argument): as qt_pose_posterior for the descriptor (but
 * frames >= 0), ld, null probs (with frames > 0), state_class, trans or carry_out, misaligned pointers (8 bytes for the
 * carries, double, int64 and the workspace), the workspace's size, an output that overlaps an input or another output; lag
 * outside 0 .. 63; negative seen or frames; frames == 0 without flush; count > 0 with a null lagged / lag_path; seen > 0 with
 * a null carry_in; carry_in overlapping carry_out.  QT_ERR_UNSUPPORTED for more than 2^20 frames in all. */
#define QT_POSE_LAG_MAX 63
typedef struct qt_pose_lag_desc {
  int batch, frames, num_classes, num_states;   /* as qt_pose_order_desc; frames = n >= 0 new frames per stream */
  int lag;                                      /* 0 .. 63 */
  int flush;                                    /* != 0: also emit the frames still pending after this call's last frame */
  long long seen;                               /* frames of every stream handed over before this call */
} qt_pose_lag_desc;
long long qt_pose_lag_smooth_carry_bytes(const qt_pose_lag_desc* desc);
long long qt_pose_lag_smooth_workspace_bytes(const qt_pose_lag_desc* desc);
int qt_pose_lag_smooth(const qt_pose_lag_desc* desc, const float* probs, long long ld, const int* state_class,
                       const int* trans, const int* init, const void* carry_in, void* carry_out, float* lagged,
                       float* lagged_class, float* filtered, double* log2_evidence, void* workspace, long long workspace_bytes,
                       void* stream);
long long qt_pose_lag_decode_carry_bytes(const qt_pose_lag_desc* desc);
long long qt_pose_lag_decode_workspace_bytes(const qt_pose_lag_desc* desc);
int qt_pose_lag_decode(const qt_pose_lag_desc* desc, const float* probs, long long ld, const int* state_class,
                       const int* trans, const int* init, const void* carry_in, void* carry_out, long long* lag_path,
                       long long* filtered, void* workspace, long long workspace_bytes, void* stream);
/* Pose-order decoding with hold durations: the best SEGMENTATION of a whole video under an explicit-duration (semi-Markov)
 * chain.  qt_pose_order_decode knows of a hold only one `stay` score per state, so every hold length is geometric and its
 * most likely length is one frame; here a segment is a pair (state, length), a table scores every length per state, and the
 * best sequence of segments is found jointly with the step order.  The reference has no such step.  Every number is an integer
 * from the emission score on, so every output is the same bits on every run.
 *
 * probs, ld, state_class, trans, init, the emission score q and e[f][j] = q(probs[f][state_class[j]]) (the floor -8192 for a
 * class outside [0, C)) are qt_pose_order_decode's; trans and init are clamped to [-65536, 0] as read.  New:
 *   dur       int32 [S][D], D = desc->max_duration in 1 .. QT_POSE_DUR_MAX = 128: dur[j][d - 1] is the score of a segment of
 *             d frames in state j, clamped to [-65536, 0] as read
 *   dur_open  int32 [S][D], or NULL for dur itself: the score of a segment that the video cuts off, which are a stream's
 *             first and last segment (a caller fills it with the suffix maximum of dur, so that a hold whose start or end lies
 *             outside the video is not charged for being short)
 *   lengths   int32 [batch] in device memory, or NULL: stream b has T_b = lengths[b] frames, clamped into 1 .. frames as
 *             read and never used as an unchecked index; NULL: every stream has `frames`
 * Forward, per stream of T frames, in exact integers (int64); cum[f][j] = the sum of e[g][j] over g < f:
 *   beta[0][j]  = max_i (init[i] + trans[i][j])        (init all zeros when NULL: the decoder's scores before the first frame)
 *   alpha[f][j] = max over d = 1 .. min(D, f) of  beta[f - d][j] + len(j, d, f) + cum[f][j] - cum[f - d][j],   f = 1 .. T
 *                 len(j, d, f) = dur_open[j][d - 1] where the segment touches a cut (f - d == 0 or f == T), else dur[j][d - 1]
 *   dlen[f][j]  = the LOWEST d that attains it
 *   beta[f][j]  = max_i (alpha[f][i] + trans[i][j]),   from[f][j] = the LOWEST i that attains it,              f = 1 .. T - 1
 * The diagonal of trans is read like any other entry: a hold of more than D frames is several segments of one state joined by
 * trans[j][j].  End: last = the lowest j that attains max_j alpha[T][j]; score[b] = that maximum.
 * Backtrace: f = T, j = last; repeat { d = dlen[f][j]; frames f - d .. f - 1 get path = j and start = f - d; f -= d; stop at
 * f == 0; j = from[f][j] }.
 *   path    int64 [batch][frames], required        start   int64 [batch][frames], or NULL: the first frame of the segment a
 *   score   int64 [batch], or NULL                         frame lies in (f - start[f]: "held for n frames")
 * Frames at and beyond T_b get path = -1 and start = -1.  A stream alone gives the bits of the same stream in a batch, and a
 * stream with lengths[b] = L the bits of a call on its first L frames.  Nothing is carried between calls: whole videos only.
 * With D = 1 and dur all zero, path is qt_pose_order_decode's path; with dur[j][d - 1] = (d - 1) stay, trans[j][j] = stay and
 * dur_open NULL, score is the decoder's best score for every D.
 * One launch, one workgroup per stream walking its frames in order: the last D rows of g[f][j] = beta[f][j] - cum[f][j] are a
 * ring of int64 in LDS (alpha[f][j] = cum[f][j] + max_d (g[f - d][j] + len)), the candidates of both maxima are spread over
 * the workgroup, and (dlen - 1) | from << 7 goes to the workspace as 16 bits per (f, j); the same workgroup then walks the
 * segments back and writes each one's frames across its lanes.  qt_pose_duration_workspace_bytes: batch * frames * S * 2,
 * rounded up to 8 bytes (every slot that is read is written in the same call), 0 for a descriptor that would be refused.  No
 * workgroup waits for another, no atomics, no host synchronisation; inputs are never written.
 *
 * qt_pose_duration_count gathers the run lengths of state paths (this decoder's, qt_pose_order_decode's, or labelled steps) for
 * fitting dur: path int64 [batch][frames] with row stride ld_path >= frames, lengths as above.  A run is a maximal stretch of
 * one state j in [0, S) over frames [s, e) of a stream's first T_b frames; an entry outside [0, S) ends a run and counts
 * nowhere.  Every run with s > 0 and e < T_b (the first and the last are cut by the video) adds 1 to
 * counts[j][min(e - s, D) - 1]; counts int64 [S][D] is added to, the caller zeroes it once.  Integer atomics: the same bits in
 * any order.  desc->num_classes is not read beyond its range check.
 *
 * QT_ERR_INVALID_ARG (before any device call, qt_last_error names the argument) for a null desc, non-positive batch or frames,
 * num_states or num_classes outside 1 .. 64, max_duration outside 1 .. 128, ld < C, ld_path < frames, a null probs,
 * state_class, trans, dur or path (count: path or counts), misaligned pointers (4 bytes for f32 and int32, 8 for int64 and
 * the workspace), a workspace smaller than the query's size, an output (path, start, score, workspace; counts) that overlaps
 * an input or another output; QT_ERR_UNSUPPORTED for more than 2^20 frames in all (batch * frames). */
#define QT_POSE_DUR_MAX 128
typedef struct qt_pose_duration_desc {
  int batch;                        /* streams */
  int frames;                       /* frames per stream (the longest; see lengths) */
  int num_classes;                  /* C, 1 .. 64 */
  int num_states;                   /* S, 1 .. 64 */
  int max_duration;                 /* D, 1 .. QT_POSE_DUR_MAX */
} qt_pose_duration_desc;
long long qt_pose_duration_workspace_bytes(const qt_pose_duration_desc* desc);
int qt_pose_duration_decode(const qt_pose_duration_desc* desc, const float* probs, long long ld, const int* state_class,
                            const int* trans, const int* init, const int* dur, const int* dur_open, const int* lengths,
                            long long* path, long long* start, long long* score, void* workspace, long long workspace_bytes,
                            void* stream);
int qt_pose_duration_count(const qt_pose_duration_desc* desc, const long long* path, long long ld_path, const int* lengths,
                           long long* counts, void* stream);
/* Pose-order posteriors with hold durations: the MARGINALS of the very chain that qt_pose_duration_decode maximises, by an
 * explicit-duration (semi-Markov) forward-backward over whole videos, and the expected duration counts that fit dur.  The
 * reference has no such step.  probs, ld, state_class, trans, init, dur, dur_open and lengths, their clamping, the limits
 * (S, C <= 64, D <= QT_POSE_DUR_MAX, batch * frames <= 2^20), lengths clamped into 1 .. frames, the emission integers
 * e[f][j] = q(probs[f][state_class[j]]) and the descriptor are qt_pose_duration_decode's, bit for bit.
 *
 * Scores are in bits: T[i][j] = trans / 256, Dur and DurOpen = dur / 256 and dur_open / 256 (DurOpen = Dur when dur_open is
 * NULL), start = init / 256 or zeros without init.  cum[f][j] = the sum of e[g][j] over g < f, an exact int64;
 * seg(f, d, j) = (cum[f][j] - cum[f - d][j]) / 256, exact; len(j, d, f) = DurOpen[j][d - 1] where the segment [f - d, f) touches
 * a cut (f - d == 0 or f == T), else Dur[j][d - 1]; L x = log2 of the sum of 2^x.  Per stream of T frames:
 *   Bt[0][j] = L_i (start[i] + T[i][j])
 *   Al[f][j] = L_{d = 1 .. min(D, f)} (Bt[f - d][j] + len(j, d, f) + seg(f, d, j))          f = 1 .. T   (segmentations of
 *                                                                                          [0, f) that end with a hold of j)
 *   Bt[f][j] = L_i (Al[f][i] + T[i][j])                                                    f = 1 .. T - 1
 *   Z        = L_j Al[T][j]                                                                log2_evidence[stream]
 *   Be[T][j] = 0;   Be[f][i] = L_j (T[i][j] + Bs[f][j])                                    f = T - 1 .. 1
 *   Bs[f][j] = L_{d = 1 .. min(D, T - f)} (len(j, d, f + d) + seg(f + d, d, j) + Be[f + d][j])      f = T - 1 .. 0
 *   begin[f][j] = 2^(Bt[f][j] + Bs[f][j] - Z)    f = 0 .. T - 1     the probability that a hold of j begins at frame f
 *   endp[f][j]  = 2^(Al[f][j] + Be[f][j] - Z)    f = 1 .. T         the probability that a hold of j ends before frame f
 *   occ[T - 1][j] = endp[T][j];   occ[t][j] = (occ[t + 1][j] + endp[t + 1][j]) - begin[t + 1][j]     (double, descending t)
 *   posterior[t][j] = r[j] / R,   r = max(occ[t], 0),   R = the sum of r[j] in ascending j (double);   R <= 0: 1 / S
 *   class_posterior[t][c] = the sum of posterior[t][j] over state_class[j] == c, in ascending j (f32)
 *   dur_counts[j][d - 1] += the sum over f = 2 .. T - 1 and d <= min(D, f - 1) of
 *                           2^(Bt[f - d][j] + Dur[j][d - 1] + seg(f, d, j) + Be[f][j] - Z)
 * dur_counts counts the segments that the video does not cut, as qt_pose_duration_count does for hard paths; it is a double
 * [S][D] that is ADDED TO (the caller zeroes it once), a stream's terms summed in descending f and the streams' sums in ascending
 * stream order from zero.  The sum of begin[f][j] over f is the expected number of holds of step j.
 * Precision: a level (Bt, Al, Be, Bs, Z) is a double (it falls by up to 288 bits a frame, and two levels that a term combines
 * lie up to D frames apart, so no per-frame normalisation applies).  Inside an L the maximum m is taken out in double; the terms
 * 2^(x - m), their sum and log2 of the sum are f32, added to m in double.  The exponent of begin, endp and of a count's term is
 * formed in double, rounded to f32, and 2^ taken in f32; occ and dur_counts are sums in double.  The order of the additions
 * inside an L depends on S and D only, never on the batch, on other streams or on the run.  Every table in range gives finite
 * outputs: the floors -8192 and -65536 are finite, so no L is empty.
 *   posterior        f32 [batch][frames][S], or NULL      class_posterior  f32 [batch][frames][C], or NULL
 *   begin            f32 [batch][frames][S], or NULL      log2_evidence    double [batch], or NULL
 *   dur_counts       double [S][D], or NULL               (posterior and dur_counts must not both be NULL)
 * Rows at and beyond T_b are zeros.  A stream alone gives the bits of the same stream in a batch, a stream with lengths[b] = L
 * the bits of a call on its first L frames, and every run the same bits.  Nothing is carried between calls: whole videos only.
 * One launch of qt_pose_duration_decode's walk, one workgroup per stream: a forward sweep with the last D rows of
 * Bt[f][j] - cum[f][j] / 256 as a ring of doubles in LDS, Al and that row going to the workspace, then the same workgroup's
 * backward sweep with the ring reused for Be[f][j] + cum[f][j] / 256, writing begin, posterior and class_posterior of a frame
 * as it passes; with dur_counts every lane also sums the terms of its own (j, d) slots, a stream's [S][D] partial goes to the
 * workspace and a second small launch adds the partials onto dur_counts.  qt_pose_duration_posterior_workspace_bytes:
 * 8 * (2 * batch * frames * S + batch * S * D) (every slot that is read is written in the same call), 0 for a descriptor that
 * would be refused.  No workgroup waits for another, no atomics, no host synchronisation; inputs are never written.
 *
 * QT_ERR_INVALID_ARG (before any device call, qt_last_error names the argument) for what qt_pose_duration_decode refuses of
 * the descriptor, ld and the inputs, a null posterior together with a null dur_counts, misaligned pointers (4 bytes for f32
 * and int32, 8 for log2_evidence, dur_counts and the workspace), a workspace smaller than the query's size, an output
 * (posterior, class_posterior, begin, log2_evidence, dur_counts, workspace) that overlaps an input or another output;
 * QT_ERR_UNSUPPORTED for more than 2^20 frames in all (batch * frames). */
long long qt_pose_duration_posterior_workspace_bytes(const qt_pose_duration_desc* desc);
int qt_pose_duration_posterior(const qt_pose_duration_desc* desc, const float* probs, long long ld, const int* state_class,
                               const int* trans, const int* init, const int* dur, const int* dur_open, const int* lengths,
                               float* posterior, float* class_posterior, float* begin, double* log2_evidence,
                               double* dur_counts, void* workspace, long long workspace_bytes, void* stream);
/* The chain with hold durations learned on the device (semi-Markov Baum-Welch): trans, init and dur fitted jointly to whole
 * videos whose frames carry class probabilities only.  The expected counts under the chain's own posterior
 * (qt_pose_duration_prior_expect), the hard counts of given segmentations (qt_pose_duration_prior_count_paths) and the new
 * tables from the counts (qt_pose_duration_prior_update) are to the chain with durations what qt_pose_prior_expect /
 * _count_paths / _update are to the plain one, whose tables do not fit here: there trans[j][j] means "stay one more frame",
 * here it joins two segments of one step.  The reference has no such step.
 * E-step.  The descriptor, probs, ld, state_class, trans, init, dur, dur_open (NULL: dur), lengths, their clamping, the limits,
 * the emission integers and the levels Bt, Al, Be, Bs, Z are qt_pose_duration_posterior's, the same arithmetic in the same
 * order.  Per stream of T frames (T = T_b):
 *   xi_f[i][j]      = 2^(Al[f][i] + T[i][j] + Bs[f][j] - Z)         f = 1 .. T - 1
 *                     P(a hold of i ends before frame f and a hold of j begins at f | the video)
 *   trans_counts[i][j] += the sum over f = 1 .. T - 1 of xi_f[i][j]  (i == j included: two joined segments of one step)
 *   xi_0[i][j]      = 2^(start[i] + T[i][j] + Bs[0][j] - Z)
 *   start_counts[i] += the sum over j (ascending) of xi_0[i][j]
 *   dur_counts[j][d - 1] += qt_pose_duration_posterior's rule, unchanged (the segments that the video does not cut)
 *   totals[0] += Z;   totals[1] += T_b
 * Consequences: sum_i xi_f[i][j] = begin[f][j] for f >= 1; sum_j xi_f[i][j] = endp[f][i]; sum_i start_counts[i] = 1 per
 * stream; T = 1 adds zeros to trans_counts, T <= 2 adds zeros to dur_counts.
 *   trans_counts double [S][S], required     start_counts double [S], or NULL
 *   dur_counts   double [S][D], required     totals       double [2], required
 * All are ADDED TO (the caller zeroes them once per E-step).  Precision follows the posterior's rule: the exponent of a term,
 * (T[i][j] + Bs[f][j]) + (Al[f][i] - Z), is formed in double, rounded to f32, and 2^ taken in f32; every sum is a double.  The
 * order of the additions is fixed: a stream's terms are added in descending f, every (i, j) and (j, d) slot by one lane of
 * its own; the streams' partials are added in ascending stream order from zero by a second small launch, and that sum is added
 * onto the accumulator.  No float atomics, no zero fill of caller memory, no host synchronisation; a stream alone gives the
 * bits of that stream's partial in a batch, and every run the same bits.
 * Contract with qt_pose_duration_posterior: on the same inputs dur_counts and every stream's Z are the BITS that it returns:
 * both are one kernel, which here writes no posterior, begin or class rows and in its backward step also adds the xi of the
 * candidates it visits anyway, with Al[f][i] from the workspace row of the forward sweep.
 * qt_pose_duration_prior_workspace_bytes: 8 * (2 * batch * frames * S + batch * (S * S + S + S * D + 1)): the two level
 * arrays and the streams' partials (8-byte aligned; every slot that is read is written in the same call); 0 for a descriptor
 * that would be refused.  It serves qt_pose_duration_prior_count_paths too, which needs less.
 * Hard counts, for path int64 [batch][frames] with row stride ld_path >= frames and start int64 in the same layout or NULL
 * (qt_pose_duration_decode's two outputs, or labelled steps without start), lengths as above.  A segment begins at frame 0 and
 * at every boundary f in 1 .. T_b - 1: with start the frames with start[f] == f (the decoder's segments: a join of one step
 * with itself counts on the diagonal), without it the frames with path[f] != path[f - 1] (runs of labelled steps).
 *   at a boundary with path[f - 1] and path[f] in [0, S):   trans_counts[path[f - 1]][path[f]] += 1
 *   a segment [s, e) with s > 0 and e < T_b whose step j = path[s] is in [0, S):   dur_counts[j][min(e - s, D) - 1] += 1
 *   start_counts[path[0]] += 1 where path[0] is in [0, S) (start_counts may be NULL);   totals[1] += T_b;   totals[0] is left alone
 * An entry outside [0, S) ends a segment and counts nowhere; without start dur_counts is qt_pose_duration_count's.  Integer
 * histograms per workgroup in LDS, added in int64 and then onto the doubles: exact, the same bits in any order.
 * desc->num_classes is not read beyond its range check.
 * M-step (one launch).  trans_out and init_out: qt_pose_prior_update's rule and code from trans_counts, start_counts, allowed
 * and pseudo_count, bit for bit.  dur_allowed int32 [S][D], non-zero where a length may be learned.  For row j, in double:
 *   r[d] = dur_allowed[j][d] ? dur_counts[j][d] + dur_pseudo_count : 0;   R = sum_d r[d], ascending
 *   R > 0:   dur_out[j][d] = dur_allowed[j][d] ? q((float)(r[d] / R)) : -65536    (q: the emission score rule; a zero scores -8192)
 *   otherwise the row keeps dur_in's values.
 *   dur_open_out[j][d], where not NULL = max over d' >= d of dur_out[j][d']
 * trans_out may be trans_in itself, init_out init_in itself, dur_out dur_in itself.
 *
 * QT_ERR_INVALID_ARG (before any device call, qt_last_error names the argument): everything qt_pose_duration_posterior refuses
 * of the descriptor, ld and the inputs (count_paths: ld_path < frames, a null path); a null trans_counts, dur_counts or
 * totals; misaligned pointers (4 bytes for f32 and int32; 8 for double, int64 and the workspace); a workspace that is too
 * small; an output that overlaps an input or another output.  qt_pose_duration_prior_update: what qt_pose_prior_update
 * refuses, max_duration outside 1 .. 128, a dur_pseudo_count that is negative, NaN or infinite, a null dur_counts, dur_allowed,
 * dur_in or dur_out.  QT_ERR_UNSUPPORTED for more than 2^20 frames in all. */
long long qt_pose_duration_prior_workspace_bytes(const qt_pose_duration_desc* desc);
int qt_pose_duration_prior_expect(const qt_pose_duration_desc* desc, const float* probs, long long ld, const int* state_class,
                                  const int* trans, const int* init, const int* dur, const int* dur_open, const int* lengths,
                                  double* trans_counts, double* start_counts, double* dur_counts, double* totals,
                                  void* workspace, long long workspace_bytes, void* stream);
int qt_pose_duration_prior_count_paths(const qt_pose_duration_desc* desc, const long long* path, const long long* start,
                                       long long ld_path, const int* lengths, double* trans_counts, double* start_counts,
                                       double* dur_counts, double* totals, void* workspace, long long workspace_bytes,
                                       void* stream);
int qt_pose_duration_prior_update(int num_states, int max_duration, const double* trans_counts, const double* start_counts,
                                  const double* dur_counts, const int* allowed, const int* dur_allowed, double pseudo_count,
                                  double dur_pseudo_count, const int* trans_in, const int* init_in, const int* dur_in,
                                  int* trans_out, int* init_out, int* dur_out, int* dur_open_out, void* stream);
/* Fixed-lag pose-order decoding with hold durations, for a loop that hands over a frame or a few per call: for the frame `lag`
 * frames ago, the state and the segment start that qt_pose_duration_decode would give on the stream up to now, at a cost per
 * step that does not grow with the video.  The reference has no such step.  probs, ld, state_class, trans, init, dur, dur_open
 * (NULL: dur), the emission integers e[f][j], the clamps to [-65536, 0] and the limits (S, C <= 64, D <= QT_POSE_DUR_MAX) are
 * qt_pose_duration_decode's, bit for bit; lag in 0 .. QT_POSE_LAG_MAX, seen, flush, frames = n >= 0 (0 with flush only),
 * batch * frames <= 2^20 per call and the emitted span are the fixed-lag pair's:
 *   g0 = max(0, seen - lag),   g1 = flush ? seen + n : max(0, seen + n - lag),   count = g1 - g0
 * There is no lengths argument: all streams of a batch advance together.
 * Forward, per stream, f = the count of frames consumed since the stream's start, in exact integers (int64); cum and beta[0] as
 * in qt_pose_duration_decode:
 *   alpha[f][j]      = max over d = 1 .. min(D, f) of  beta[f - d][j] + len + cum[f][j] - cum[f - d][j],   len = dur_open[j][d - 1]
 *                      where f - d == 0 (the segment touches the stream's start), else dur[j][d - 1];   dlen[f][j] = the LOWEST
 *                      d that attains it
 *   alpha_open[f][j] = the same maximum with len = dur_open[j][d - 1] for every d, as if the stream were cut after frame f, and
 *                      dlen_open[f][j] its lowest d (dur_open NULL: alpha and dlen themselves)
 *   beta[f][j]       = max_i (alpha[f][i] + trans[i][j]),   from[f][j] = the LOWEST i: built from the closed alpha, as the
 *                      whole-video decoder does for f < T
 *   end[f]           = the LOWEST j that attains best[f] = max_j alpha_open[f][j]
 * Window of an emitted frame g (0-based), with last = seen + n - 1, w = min(g + lag, last), F = w + 1:
 *   j = end[F], d = dlen_open[F][j], f = F;  repeat { if f - d <= g: lag_path[g] = j, lag_start[g] = f - d, stop;
 *   f -= d;  j = from[f][j];  d = dlen[f][j] }
 * which reads from and dlen at g < f <= w only: at most lag rows.
 *   lag_path   int64 [batch][count], required when count > 0    lag_start  int64 [batch][count], or NULL: the global index of
 *   filtered   int64 [batch][n], or NULL: end[f] of each                   the first frame of the segment frame g lies in
 *              new frame                                        score      int64 [batch][n], or NULL: best[f] of each new frame
 * Carry.  Caller-owned device memory as two buffers that must not overlap, carry_in (read; not read and may be NULL with seen
 * == 0) and carry_out (written in full); the caller swaps them between calls.  Per stream { int64 cum[S]; int64 g[D][S]:
 * g[f][j] = beta[f][j] - cum[f][j] at row f mod D for the last D values of f, rows never written zero; uint16 hist[lag][S]:
 * (dlen - 1) | from << 7 of f = seen + n - lag + 1 + k in slot k, zeros for f <= 0; uint16 tail = (dlen_open[F][end[F]] - 1) |
 * end[F] << 7 of the newest F = seen + n (0 at F == 0; a flush with frames == 0 starts its walks there) }, rounded up to 8
 * bytes.  qt_pose_duration_lag_carry_bytes gives the size of one buffer.  lag, the tables, D and batch are fixed for the life
 * of a stream.  The scores are absolute: no offset, no saturation; seen + frames may be at most 2^36 (|beta| < 2^54).
 * Contract.  For any split of a stream into calls, flush on the last, every output and the final carry are the bits of one
 * call (one route, no environment switch).  lag_path[g] and lag_start[g] are path[g] and start[g] of qt_pose_duration_decode
 * on the stream's first min(g + lag, last) + 1 frames, score of frame f is its score on the first f + 1 frames; hence a
 * one-call flush with n <= lag + 1 is qt_pose_duration_decode on those frames.  With D == 1 and dur all zero lag_path is
 * qt_pose_lag_decode's.  A stream alone gives the bits it has in a batch.
 * One launch, one workgroup of 256 per stream, qt_pose_duration_decode's frame step with both maxima: the ring g comes from
 * carry_in into LDS (beta[0] at seen == 0), every new frame's hist row and tail word go to the workspace (uint16 [batch][n][S]
 * and [batch][n], each rounded up to 8 bytes; 0 bytes at n == 0), filtered and score are written per frame, and behind a
 * barrier one thread per emitted frame walks its window through the workspace (the workgroup's own stores) and carry_in's
 * hist; then carry_out.  qt_pose_duration_lag_workspace_bytes: what the call needs, 0 for a descriptor that would be refused
 * (as the carry query).  No atomics, no host synchronisation, no workgroup waits for another; inputs, carry_in included, are
 * never written; every workspace slot that is read is written in the same call.
 *
 * QT_ERR_INVALID_ARG (before any device call, qt_last_error names the argument): the descriptor's ranges (batch >= 1, frames
 * >= 0, num_classes and num_states in 1 .. 64, max_duration in 1 .. 128, lag in 0 .. 63, seen >= 0), ld < C, a null probs
 * (with frames > 0), state_class, trans, dur or carry_out, count > 0 with a null lag_path, seen > 0 with a null carry_in,
 * frames == 0 without flush, misaligned pointers (4 bytes for f32 and int32; 8 for int64, the carries and the workspace), a
 * workspace smaller than the query's size, an output that overlaps an input or another output (carry_in overlapping
 * carry_out included).  QT_ERR_UNSUPPORTED for more than 2^20 frames in a call (batch * frames) and for seen + frames > 2^36. */
typedef struct qt_pose_duration_lag_desc {
  int batch, frames, num_classes, num_states;   /* as qt_pose_lag_desc; frames = n >= 0 new frames per stream */
  int max_duration;                             /* D, 1 .. QT_POSE_DUR_MAX */
  int lag;                                      /* 0 .. QT_POSE_LAG_MAX */
  int flush;                                    /* != 0: also emit the frames still pending after this call's last frame */
  long long seen;                               /* frames of every stream handed over before this call */
} qt_pose_duration_lag_desc;
long long qt_pose_duration_lag_carry_bytes(const qt_pose_duration_lag_desc* desc);
long long qt_pose_duration_lag_workspace_bytes(const qt_pose_duration_lag_desc* desc);
int qt_pose_duration_lag_decode(const qt_pose_duration_lag_desc* desc, const float* probs, long long ld,
                                const int* state_class, const int* trans, const int* init, const int* dur, const int* dur_open,
                                const void* carry_in, void* carry_out, long long* lag_path, long long* lag_start,
                                long long* filtered, long long* score, void* workspace, long long workspace_bytes,
                                void* stream);
/* Fixed-lag pose-order posteriors with hold durations, for a loop that hands over a frame or a few per call: for the frame `lag`
 * frames ago, the row of posterior, class_posterior and begin that qt_pose_duration_posterior would give on the stream up to
 * now, and for every new frame the lag-0 row and the evidence, at a cost per step that does not grow with the video.  The
 * reference has no such step.
 * From qt_pose_duration_lag_decode, unchanged, bit for bit: the descriptor qt_pose_duration_lag_desc, lag, seen, flush,
 * frames = n >= 0 (0 with flush only), batch * frames <= 2^20 per call, the emitted span
 *   g0 = max(0, seen - lag),   g1 = flush ? seen + n : max(0, seen + n - lag),   count = g1 - g0
 * the two caller-owned carry buffers that are swapped between calls, and no lengths argument: all streams advance together.
 * From qt_pose_duration_posterior, unchanged, bit for bit: probs, ld and the tables with their clamps, the emission integers
 * e[f][j], T, Dur, DurOpen (Dur when dur_open is NULL) and start in bits, cum and seg, the levels as doubles, the L rule (the
 * maximum taken out in double; the terms 2^(x - m), their sum and log2 of the sum f32), and the precision of begin, endp (the
 * exponent formed in double, rounded to f32, 2^ in f32) and occ (double).
 * Forward, per stream, f = the count of frames consumed since the stream's start:
 *   Bt[0][j]      = L_i (start[i] + T[i][j])
 *   Al[f][j]      = L_{d = 1 .. min(D, f)} (Bt[f - d][j] + len + seg(f, d, j)),   len = DurOpen[j][d - 1] where f - d == 0 (the
 *                   segment touches the stream's start), else Dur[j][d - 1]: the closed level, what qt_pose_duration_posterior
 *                   computes for f < T
 *   Al_open[f][j] = the same L with len = DurOpen[j][d - 1] for every d, as if the stream were cut after frame f: that
 *                   kernel's Al[T] at T = f (dur_open NULL: Al itself)
 *   Bt[f][j]      = L_i (Al[f][i] + T[i][j]): always from the closed Al
 *   Z_f           = L_j Al_open[f][j], in ascending j
 * Window of an emitted frame g (0-based), with last = seen + n - 1 and F = min(g + lag, last) + 1: the posterior's backward
 * sweep on the prefix [0, F), from f = F - 1 down to f = g only:
 *   Be[F][j] = 0
 *   Bs[f][j] = L_{d = 1 .. min(D, F - f)} (len(j, d, f + d) + seg(f + d, d, j) + Be[f + d][j]),   DurOpen where f + d == F or f == 0
 *   Be[f][i] = L_j (T[i][j] + Bs[f][j])                                           f > g
 *   begin[f][j] = 2^(Bt[f][j] + Bs[f][j] - Z_F)
 *   endp[f][j]  = 2^(Al[f][j] + Be[f][j] - Z_F)   f < F;     endp[F][j] = 2^(Al_open[F][j] - Z_F)
 *   occ[F - 1][j] = endp[F][j];   occ[t][j] = (occ[t + 1][j] + endp[t + 1][j]) - begin[t + 1][j]     (double, descending t)
 *   lagged[g][j]       = r[j] / R,   r = max(occ[g], 0),   R = the sum of r[j] in ascending j (double);   R <= 0: 1 / S
 *   lagged_class[g][c] = the sum of lagged[g][j] over state_class[j] == c, in ascending j (f32)
 *   lagged_begin[g][j] = begin[g][j]: the probability that a hold of j begins at frame g, given lag frames of look-ahead
 * which reads Bt[f] at g <= f < F, Al[f] at g < f <= F and the emissions of frames g .. F - 1: at most lag + 1 rows, however
 * old the stream is.  Per new frame f = seen + 1 .. seen + n: filtered[f - 1] is the row that the window (g = f - 1, F = f)
 * gives, the lag-0 answer, and log2_evidence[f - 1] = Z_f.
 *   lagged         f32 [batch][count][S], required when count > 0     lagged_class   f32 [batch][count][C], or NULL
 *   lagged_begin   f32 [batch][count][S], or NULL                     filtered       f32 [batch][n][S], or NULL
 *   log2_evidence  double [batch][n], or NULL
 * Carry.  carry_in (read; not read and may be NULL with seen == 0) and carry_out (written in full, the padding zero) must not
 * overlap.  Per stream, with end = seen + n of the call that writes it: { int64 cum[S] = cum[end]; double ring[D][S]:
 * Bt[f][j] - cum[f][j] / 256 at row f mod D for the last D values of f, rows never written zero; double gh[lag][S]: the same
 * quantity of f = end - lag + k in slot k; double al[lag][S]: the closed Al[f] of f = end - lag + 1 + k; double al_open[S] and
 * double Z: Al_open[end] and Z_end (a flush with frames == 0 starts its windows there; zeros at end == 0); int16 e[lag][S]: the
 * emissions of frame end - lag + k }, rounded up to 8 bytes: 8 S + 8 D S + 16 lag S + 8 S + 8 + 2 lag S.  Slots of frames in
 * front of the stream's start (f < 0; f <= 0 for al) are zeros.  qt_pose_duration_lag_smooth_carry_bytes gives the size of one
 * buffer.  lag, the tables, D and batch are fixed for the life of a stream.
 * Levels are absolute doubles, as in the whole-video kernel (which is what lets the bits agree); they lose an ulp of a bit per
 * 2^20 frames or so at 288 bits a frame, so seen + frames may be at most 2^20, that kernel's own limit (9.7 hours at 30 fps).
 * Contract.  (1) lagged[g], lagged_class[g] and lagged_begin[g] are the BITS of row g of posterior, class_posterior and begin
 * of qt_pose_duration_posterior on the stream's first F frames; log2_evidence of frame f - 1 is the bits of its log2_evidence
 * on the first f frames.  (2) For any split of a stream into calls, flush on the last, every output and the final carry are
 * the bits of one call (one route, no environment switch); a stream alone gives the bits it has in a batch; every run gives
 * the same bits.  Hence: lag == 0 makes lagged the rows of filtered; a one-call flush of n <= lag + 1 frames is
 * qt_pose_duration_posterior on them; with D == 1 and dur all zero lagged is the plain chain's lagged posterior
 * (qt_pose_lag_smooth's rule, up to f32 rounding).
 * Two launches.  The first, one workgroup of 256 per stream, is qt_pose_duration_posterior's forward step with both Ls over
 * the same ring rows, the ring from carry_in (Bt[0] at seen == 0); every new frame's row of Bt - cum / 256, closed Al,
 * Al_open, cum (double, double, double, int64 [batch][n][S] each), Z_f (double [batch][n]) and int16 emissions ([batch][n][S],
 * rounded up to 8 bytes) go to the workspace; it writes log2_evidence and then carry_out.  The second, one workgroup per
 * (stream, emitted frame) and with filtered per (stream, new frame), sweeps its window with the same lane map, so that an L
 * adds in the posterior's order, which depends on S and D alone; it reads the workspace for the frames of this call and
 * carry_in for older ones and writes its one row of each output.  Windows share nothing, so a window's bits cannot depend on
 * the split.  qt_pose_duration_lag_smooth_workspace_bytes: 32 batch n S + 8 batch n + 2 batch n S rounded up to 8; 0 at n == 0
 * and for a descriptor that would be refused (as the carry query).  No atomics, no host synchronisation, no workgroup waits
 * for another; inputs, carry_in included, are never written; every workspace slot that is read is written in the same call.
 *
 * QT_ERR_INVALID_ARG (before any device call, qt_last_error names the argument): what qt_pose_duration_lag_decode refuses,
 * with lagged in the place of lag_path; misaligned pointers (4 bytes for f32 and int32; 8 for log2_evidence, the carries and
 * the workspace); an output (carry_out, lagged, lagged_class, lagged_begin, filtered, log2_evidence, workspace) that overlaps
 * an input or another output (carry_in overlapping carry_out included).  QT_ERR_UNSUPPORTED for more than 2^20 frames in a
 * call (batch * frames) and for seen + frames > 2^20. */
long long qt_pose_duration_lag_smooth_carry_bytes(const qt_pose_duration_lag_desc* desc);
long long qt_pose_duration_lag_smooth_workspace_bytes(const qt_pose_duration_lag_desc* desc);
int qt_pose_duration_lag_smooth(const qt_pose_duration_lag_desc* desc, const float* probs, long long ld,
                                const int* state_class, const int* trans, const int* init, const int* dur, const int* dur_open,
                                const void* carry_in, void* carry_out, float* lagged, float* lagged_class, float* lagged_begin,
                                float* filtered, double* log2_evidence, void* workspace, long long workspace_bytes,
                                void* stream);
/* Data-gradient operand of a stride-2 conv (k = 3 pad 1, or k = 1 pad 0) split by the parity
 * (ph, pw) of the input pixel: class c = ph*2+pw gets [I][taps_c][O] with only the taps that
 * reach it (k=3: 1,2,2,4 taps; k=1: 1,0,0,0), stored back to back in class order.  Row taps of
 * class parity 0: {1}; parity 1: {2, 0} (source row i, i+1).  Element offsets of the four
 * classes are returned in class_offset[4], tap grid in class_kh[4] / class_kw[4] (host arrays). */
int qt_pack_dgrad_s2(int dtype, const float* w_oihw, void* dst, int O, int I, int k, long long* class_offset,
                     int* class_kh, int* class_kw, void* stream);
/* The same four classes as ONE operand [4*I][2*2][O] for a single 2x2-tap launch over the gradient map
 * (qt_conv_desc.dst_merge = I, kh = kw = 2, pad 0, n_out = 4*I): row class*I + i, tap slot th*2 + tw with th / tw = 0
 * the tap on the source row / column itself, 1 the tap on the next one; slots no tap maps to are zero.  k = 3 only;
 * dst holds 16*O*I elements (9/16 of them non-zero: the launch reads the gradient map once instead of four times and
 * needs no per-class launches, at 16/9 of the MFMA work). */
int qt_pack_dgrad_s2_merged(int dtype, const float* w_oihw, void* dst, int O, int I, void* stream);
/* [64][3][7][7] -> [64][taps][8][4] for the packed stem; taps = 7, or 8 (8th row zero)
 * when a 32-element tap is only half a K-step (bf16: desc.kh = 8) */
int qt_pack_stem_weight(int dtype, const float* w_oihw, void* dst, int taps, void* stream);
/* [O][kh][kw][I] f32 gradient -> OIHW f32 (.grad), optionally accumulating */
int qt_unpack_conv_wgrad(const float* dw, float* grad_oihw, int O, int I, int kh, int kw, int accumulate, void* stream);
int qt_unpack_stem_wgrad(const float* dw, float* grad_oihw, int accumulate, void* stream);

/* ------------------------------------------------------------------------
 * BatchNorm2d (torch defaults eps 1e-5, momentum 0.1; replaces nn.BatchNorm2d of
 * torchvision's ResNet-18 in train() and eval() mode) and fused activations.
 * ------------------------------------------------------------------------ */
/* partial[rows][2][C] (from qt_conv2d_igemm) -> batch mean / invstd, scale = gamma*invstd,
 * shift = beta - mean*scale; updates running stats (unbiased var) if given. */
/* partial buffers must have room for qt_stats_capacity_rows(rows) rows (long row
 * counts are folded 256:1 into the spare rows before the final reduction). */
int qt_stats_capacity_rows(int rows);
int qt_bn_finalize(float* partial, int rows, int C, long long count, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps,
                   float* mean, float* invstd, float* scale, float* shift, void* stream);
/* eval mode: scale/shift from running statistics */
int qt_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                      float eps, int C, float* scale, float* shift, void* stream);
/* the same for up to 32 BatchNorms in one launch (an eval forward needs all of them up front) */
typedef struct qt_bn_eval_item {
  const float *gamma, *beta, *running_mean, *running_var;
  float *scale, *shift;
  int C;
  float *mean, *invstd; /* optional pair: running_mean and 1/sqrt(running_var + eps), what the backward kernels read */
} qt_bn_eval_item;
int qt_bn_eval_affine_batched(const qt_bn_eval_item* items, int n, float eps, void* stream);
/* out = relu?( y*scale+shift + (residual ? residual*res_scale+res_shift : 0) ), [M][C] */
int qt_bn_act(int dtype, const void* y, const float* scale, const float* shift, const void* residual,
              const float* res_scale, const float* res_shift, int relu, void* out, long long M, int C, void* stream);
/* the same, and mask_bits (nullable) receives out > 0 as one bit per element: [M][C/8] bytes, bit (c & 7) of byte c / 8 --
 * the ReLU mask in the form qt_conv_io.relu_mask_bits takes (the training forward of the plan writes it for every
 * activation whose mask a data-gradient epilogue applies) */
int qt_bn_act_mask(int dtype, const void* y, const float* scale, const float* shift, const void* residual,
                   const float* res_scale, const float* res_shift, int relu, void* out, unsigned char* mask_bits,
                   long long M, int C, void* stream);
/* backward: g = d(loss)/d(BN output) (masked by `mask` > 0 if given).  qt_bn_bwd_finalize with count == 0 is the backward of
 * an eval-mode BatchNorm (running statistics in mean / invstd): dx = g*gamma*invstd without the batch-mean terms. */
/* qt_bn_bwd_partial_rows: rows qt_bn_bwd_reduce writes, or QT_ERR_INVALID_ARG for the channel counts it refuses (C a multiple of 8,
 * at most 2048, with C / 8 dividing 256) */
int qt_bn_bwd_partial_rows(long long M, int C);
int qt_bn_bwd_reduce(int dtype, const void* g, const void* mask, const void* y, const float* mean, const float* invstd,
                     float* partial, long long M, int C, void* stream);
int qt_bn_bwd_finalize(float* partial, int rows, int C, long long count, const float* gamma, const float* invstd,
                       float* dgamma, float* dbeta, int accumulate, float* coef /*[3][C]*/, void* stream);
int qt_bn_bwd_apply(int dtype, const void* g, const void* mask, const void* y, const float* mean, const float* invstd,
                    const float* coef, void* dy, void* g_out, long long M, int C, void* stream);

/* stem: relu(y*scale+shift) then MaxPool2d(3,2,1): [B][112][112][64] -> [B][56][56][64]
 * (torchvision bn1/relu/maxpool, Quadtree_from scratch/models.py:224-226); argmax (u8, optional)
 * records the winning tap for the backward, y_at_max (optional, same shape and type as pooled)
 * the raw conv1 output at that tap (input of qt_stem_bn_bwd_sums). */
int qt_stem_pool(int dtype, const void* y, const float* scale, const float* shift, void* pooled,
                 unsigned char* argmax, void* y_at_max, int batch, void* stream);
/* Eval forward: conv1 (packed stem descriptor: xpad, qt_pack_stem_weight's [64][taps][32]) + folded BatchNorm
 * (scale / shift) + ReLU + MaxPool2d(3,2,1) in one launch; the conv1 map never reaches memory.  bf16 only
 * (QT_ERR_UNSUPPORTED otherwise: qt_conv2d_igemm + qt_stem_pool). */
int qt_stem_conv_pool(int dtype, const void* xpad, const void* weight, int taps, const float* scale, const float* shift,
                      void* pooled, int batch, void* stream);
/* The same straight from the f32 NCHW image [B][3][224][224] the reference's dataloader hands over (16-byte aligned): the
 * kernel packs its input rows in LDS (same rounding as qt_pack_stem_input), so neither xpad nor the conv1 map exists in
 * memory; bit-identical to qt_pack_stem_input + qt_stem_conv_pool.  QT_ERR_UNSUPPORTED (take the packed form) for f32, an
 * image that is not 16-byte aligned, or QTCNN_STEM_NCHW=0. */
int qt_stem_conv_pool_nchw(int dtype, const float* image_nchw, const void* weight, int taps, const float* scale,
                           const float* shift, void* pooled, int batch, void* stream);
int qt_stem_pool_bwd(int dtype, const void* dpooled, const unsigned char* argmax, const void* y, const float* scale,
                     const float* shift, void* g, int batch, void* stream);
/* The same gradient fused with bn1's backward, without materialising it: _reduce emits
 * qt_stem_bn_bwd_rows(batch) rows of partial sums for qt_bn_bwd_finalize, _apply writes
 * d(loss)/d(conv1 output) directly. */
int qt_stem_bn_bwd_rows(int batch);
int qt_stem_bn_bwd_reduce(int dtype, const void* dpooled, const unsigned char* argmax, const void* y,
                          const float* scale, const float* shift, const float* mean, const float* invstd,
                          float* partial, int batch, void* stream);
/* The same partial sums from the pooled side (each pooled cell feeds one conv1 position): reads
 * dpooled and y_at_max only.  qt_stem_bn_bwd_sums_rows(batch) rows. */
int qt_stem_bn_bwd_sums_rows(int batch);
int qt_stem_bn_bwd_sums(int dtype, const void* dpooled, const void* y_at_max, const float* scale, const float* shift,
                        const float* mean, const float* invstd, float* partial, int batch, void* stream);
int qt_stem_bn_bwd_apply(int dtype, const void* dpooled, const unsigned char* argmax, const void* y, const float* scale,
                         const float* shift, const float* mean, const float* invstd, const float* coef, void* dy,
                         int batch, void* stream);
/* Stem backward in one launch (bf16): the gradient of conv1's output (max-pool backward + ReLU mask + BatchNorm backward,
 * the arithmetic of qt_stem_bn_bwd_apply) is computed tile by tile in LDS and contracted with the packed input at once:
 * dw[64][7][32] (the layout qt_unpack_stem_wgrad reads, zeroed by the caller) += conv1's weight gradient.  The 411 MB map
 * d(loss)/d(conv1 output) is neither written nor read.  Each workgroup writes its partial filter to `workspace`
 * (qt_stem_bn_bwd_wgrad_workspace_bytes(batch)) and a second launch adds them to dw in workgroup order: the same bits on
 * every run.  QT_ERR_UNSUPPORTED for f32 / QTCNN_STEM_BWD_FUSED=0: use qt_stem_bn_bwd_apply + qt_conv2d_wgrad. */
size_t qt_stem_bn_bwd_wgrad_workspace_bytes(int batch);
int qt_stem_bn_bwd_wgrad_ws(int dtype, const void* dpooled, const unsigned char* argmax, const void* y, const float* scale,
                            const float* shift, const float* mean, const float* invstd, const float* coef, const void* xpad,
                            float* dw, void* workspace, size_t workspace_bytes, int batch, void* stream);
/* Data gradient of conv1 down to the image: dx [B][3][224][224] f32 NCHW (written, not accumulated) =
 * conv_transpose2d(dy, w, stride 2, padding 3) from dy = d(loss)/d(conv1 output) [B][112][112][64] in `dtype` (bf16 or
 * f32; 16-byte aligned) and conv1's f32 OIHW master weight [64][3][7][7].  One MFMA GEMM over 2 x 2 image blocks
 * (K = 4 x 4 dy positions x 64 channels, N = 3 channels x 4 parities); the bf16 build splits the weight into two bf16
 * halves, so dy's own rounding is the only one.  QT_ERR_UNSUPPORTED for any other dtype or alignment. */
int qt_stem_dgrad(int dtype, const void* dy, const float* w_oihw, float* dx, int batch, void* stream);
/* AdaptiveAvgPool2d(1,1)+flatten into columns [col0, col0+C) of the fused feature
 * matrix (Quadtree_from scratch/models.py:242,289-294) and its backward fused with the
 * ReLU mask of the pooled map. */
int qt_avgpool(int dtype, const void* x, void* dst, int batch, int hw, int C, int ld, int col0, void* stream);
int qt_avgpool_bwd(int dtype, const void* d, const void* x, void* g, int batch, int hw, int C, int ld, int col0,
                   void* stream);
/* quadrant head tail: MaxPool2d(2,2) (7->3) + flatten(1) + torch.cat placement
 * (Quadtree_from scratch/models.py:237,284-294): q [B*4][7][7][128] -> dst[b][col0 + quad*1152 + c*9 + ph*3 + pw] */
int qt_quad_pool(int dtype, const void* q, void* dst, int batch, int ld, int col0, void* stream);
int qt_quad_pool_bwd(int dtype, const void* d, const void* q, void* dq, int batch, int ld, int col0, void* stream);
/* Heads of AttentionHierarchicalCNN (Quadtree_from scratch/models.py:6-101).
 * qt_region_avgpool: AdaptiveAvgPool2d((1,1)) + flatten of the per-region conv+ReLU maps x [batch*split^2][hw][C]
 *   (:21-30) into dst[b*ld + col0 + slot*C + c]; `slot` is the reference's append order -- quadrants TL,TR,BL,BR
 *   (:62-67), and for split 4 quadrant*4 + sub-quadrant (:70-78).  dst_dtype: `dtype` or QT_F32.
 * qt_region_avgpool_bwd: g = x > 0 ? d[...]/hw : 0  (mean-pool backward fused with the ReLU mask).
 * qt_attention_gate (:34-38,:81-89): v [B][16][64] f32; act [B][16][32] = relu(W1 v + b1); alpha [B][16] =
 *   softmax_j(w2 . act_j + b2); out[b*ld + col0 + c] = sum_j alpha_j v_j[c]   (out has type `dtype`).
 * qt_attention_gate_bwd: from d[b*ld + col0 + c] -> dv [B][16][64], and the two row-wise factors of the
 *   parameter gradients: ds [B][16] (d/d score) and dpre [B][16][32] (d/d pre-ReLU hidden), so that
 *   dW1 = dpre^T v, db1 = sum dpre, dw2 = ds^T act, db2 = sum ds (qt_gemm_small / qt_col_sum).
 * qt_relu_mask_cols: out[r][c] = act[r*ld+col0+c] > 0 ? d[r*ld+col0+c]*mul : 0  (f32, dense): backward of the
 *   Linear -> ReLU -> Dropout numerical branch (:43-46) whose output lives inside the fused feature matrix. */
int qt_region_avgpool(int dtype, const void* x, void* dst, int dst_dtype, int batch, int split, int hw, int C, int ld,
                      int col0, void* stream);
int qt_region_avgpool_bwd(int dtype, const void* d, int d_dtype, const void* x, void* g, int batch, int split, int hw,
                          int C, int ld, int col0, void* stream);
int qt_attention_gate(int dtype, const float* v, const float* w1, const float* b1, const float* w2, const float* b2,
                      float* act, float* alpha, void* out, int batch, int ld, int col0, void* stream);
int qt_attention_gate_bwd(int dtype, const void* d, const float* v, const float* act, const float* alpha, const float* w1,
                          const float* w2, float* ds, float* dpre, float* dv, int batch, int ld, int col0, void* stream);
int qt_relu_mask_cols(int dtype, const void* d, const void* act, float* out, long long rows, int cols, int ld, int col0,
                      float mul, void* stream);
/* nn.LSTM recurrence (cnn+lstm/models.py:43-49,81-86; batch_first, one direction, f32, torch gate order i,f,g,o).
 * qt_lstm_forward: xproj [B][T][4H] = x_t W_ih^T + b_ih for every step (a thin product done by the caller; b_hh
 *   [4H], nullable, is added here),
 *   whh_t = W_hh^T [H][4H] (qt_transpose_f32) -> gates [B][T][4H] (post-activation), cell / hprev / hout [B][T][H]
 *   (hprev = h_{t-1}, zeros at t = 0).  One launch, one workgroup per sequence; H in {256, 64}.
 * qt_lstm_backward: dhout [B][T][H] (gradient w.r.t. every h_t, nullable) + dlast [B][H] (w.r.t. h_{T-1}, nullable)
 *   -> dgates [B][T][4H] w.r.t. the pre-activation gates; then dx = dgates W_ih, dW_ih = dgates^T x,
 *   dW_hh = dgates^T hprev, db_ih = db_hh = column sums (qt_gemm_small / qt_col_sum).  whh = W_hh [4H][H].
 * qt_scale_by_nonzero: g = x != 0 ? g*mul : 0 -- backward of the dropout between LSTM layers from the dropped
 *   activations themselves. */
int qt_lstm_forward(const float* xproj, const float* whh_t, const float* bhh, float* gates, float* cell, float* hprev,
                    float* hout, int batch, int T, int H, void* stream);
int qt_lstm_backward(const float* dhout, const float* dlast, const float* gates, const float* cell, const float* whh,
                     float* dgates, int batch, int T, int H, void* stream);
int qt_transpose_f32(const float* src, float* dst, int rows, int cols, void* stream);
int qt_scale_by_nonzero(float* g, const float* x, long long n, float mul, void* stream);
/* dst[i] = (float)src[i] (src of type `dtype`): f32 copy of the fused per-frame features for the f32 LSTM products */
int qt_cast_f32(int dtype, const void* src, float* dst, long long n, void* stream);
/* The same 2-layer LSTM on a video STREAM: one row of h1 per frame instead of one per materialised window.
 * The rule.  S streams advance together by n >= 1 frames per call; `seen` frames came before the call.  Frame f of the
 *   call has global index g = seen + f and gets one row: h1 at the last step of the 2-layer LSTM run from a zero state
 *   over the len = min(T, g + 1) frames ending at g, eval arithmetic (no dropout between the layers).  For g >= T - 1
 *   that is the model in eval() on the materialised window, for the first T - 1 frames of a stream the model at sequence
 *   length g + 1: as many rows as have been seen, the rule of qt_timeline_smooth.
 * qt_lstm_stream_forward: xproj0 [S][T-1+n][4H] = layer 0's input products x W_ih0^T + b_ih0, ONE row per frame: the
 *   T - 1 carry rows (the frames before the call) first, then the call's n rows; window f reads rows f .. f+T-1, and
 *   rows of frames in front of the stream's start (row r with seen - (T-1) + r < 0) are never read, whatever they hold.
 *   whh0_t / wih1_t / whh1_t = W_hh0^T / W_ih1^T / W_hh1^T, each [H][4H] (qt_transpose_f32); bhh0 / bih1 / bhh1 [4H].
 *   -> hlast [S][n][H], and carry_out [S][T-1][4H] (nullable; must not be xproj0's storage: the caller swaps two
 *   buffers) = the last T - 1 rows of xproj0, rows in front of the stream's start as zeros.  One launch runs both
 *   layers, layer 1's input product included; a workgroup owns QT_LSTM_STREAM_TILE consecutive windows of one stream (one
 *   window when n == 1, the live step) and reads every weight matrix once per step for the tile.  No buffer of size windows x T exists: the workspace
 *   (qt_lstm_stream_workspace_bytes, the caller's) is 0 bytes today and may be NULL.  f32, no atomics, no host sync.
 *   Every window is its own k-ordered fmaf chains, so its bits do not depend on its place in a tile, on n or on S: any
 *   split of a stream into consecutive calls gives the hlast and the final carry of one call, and a stream alone the
 *   bits it has in a batch.  H in {256, 64}, 1 <= T <= 64, else QT_ERR_UNSUPPORTED before any launch; all operands
 *   16-byte aligned.
 * qt_lstm_stream_stage: xproj0 [S][T-1+n][4H] <- carry_in [S][T-1][4H] (NULL when T == 1) in front of xnew [S][n][4H]
 *   (the dense product of the call's frames); same limits. */
#define QT_LSTM_STREAM_TILE 8
size_t qt_lstm_stream_workspace_bytes(int S, int n, int T, int H);
int qt_lstm_stream_forward(const float* xproj0, const float* whh0_t, const float* bhh0, const float* wih1_t,
                           const float* bih1, const float* whh1_t, const float* bhh1, float* hlast, float* carry_out,
                           void* workspace, size_t workspace_bytes, long long seen, int S, int n, int T, int H, void* stream);
int qt_lstm_stream_stage(const float* carry_in, const float* xnew, float* xproj0, int S, int n, int T, int H, void* stream);
/* nn.Dropout (Quadtree_from scratch/models.py:258,269), in place, counter-hash RNG */
int qt_dropout(int dtype, void* x, long long rows, int cols, int ld, unsigned long long seed, float p, void* stream);
/* g = act > 0 ? g*mul : 0 (ReLU / dropout backward from the forward output) */
int qt_relu_mask_scale(int dtype, void* g, const void* act, long long n, float mul, void* stream);
/* out[c] (+)= sum_r x[r*ld+c]  (bias gradients) */
int qt_col_sum(int dtype, const void* x, long long rows, int cols, int ld, float* out, int accumulate, void* stream);
/* The same, deterministic: row chunks (at most 1024) write their column sums to `workspace` (qt_col_sum_workspace_bytes), a
 * second launch adds them in chunk order (qt_col_sum's atomics depend on the order the chunks finish in once there are more
 * than two) */
size_t qt_col_sum_workspace_bytes(long long rows, int cols);
int qt_col_sum_ws(int dtype, const void* x, long long rows, int cols, int ld, float* out, int accumulate, void* workspace,
                  size_t workspace_bytes, void* stream);

/* nn.Linear on a small batch with a large weight matrix (classifier.0: Linear(5376 -> 2688) + ReLU,
 * Quadtree_from scratch/models.py:266-268, and its backward-input product), bf16:
 *   y[m][n] = relu?( bias[n] + sum_k x[m][k] * w[n][k] ),  x [M][K], w [N][K], y [M][N]
 * split over K so that every CU streams a disjoint block of the weights once; partial products go
 * through `workspace` (qt_linear_workspace_bytes, f32 [S][M][N]) and are added in a fixed order.
 * Covers M <= 256, N % 64 == 0, K % 64 == 0; anything else returns QT_ERR_UNSUPPORTED (use
 * qt_conv2d_igemm with a 1x1 descriptor). */
size_t qt_linear_workspace_bytes(int M, int N, int K);
int qt_linear_bf16(const void* x, const void* w, const float* bias, int relu, void* y, int M, int N, int K,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Thin dense products (nn.Linear 47->94->256 and 2688->12 and their gradients,
 * Quadtree_from scratch/models.py:255-260,270): C[m][n] = relu?(acc? + bias[n] +
 * sum_k A[m*ars+k*aks] * B[n*brs+k*bks]).
 * ------------------------------------------------------------------------ */
typedef struct qt_gemm_small_desc {
  int M, N, K;
  int a_dtype, b_dtype, c_dtype;
  long long a_row_stride, a_k_stride;
  long long b_row_stride, b_k_stride;
  long long c_row_stride;
  int relu, accumulate;
} qt_gemm_small_desc;
int qt_gemm_small(const qt_gemm_small_desc* desc, const void* A, const void* B, const float* bias, void* C,
                  void* stream);

/* ------------------------------------------------------------------------
 * 3-D clip models (Quadtree3DCNN 3dcnn/models.py:96-214, Ji3DCNN cnn+lstm/models.py:93-142).  Clip activations are
 * time-major NHWC [T][B][H][W][C]: a Conv3d(3x3x3, padding 1) is three qt_conv2d_igemm launches over contiguous frame
 * ranges (out[t] += conv2d(in[t+kt-1], W[:,:,kt]), accumulated through `residual` = dst), its gradients three
 * QT_CONV_DGRAD / qt_conv2d_wgrad launches (host side: <pkg>/video3d.py).  The HBM-bound pieces:
 * ------------------------------------------------------------------------ */
/* clips [B][T][3][H][W] f32 (the reference's image_sequence_input) -> [T][B][H][W][128] of `dtype`: the 27 taps x 3
 * channels of pixel (t,b,h,w), element ((kt*3+kh)*3+kw)*3+c, zeros outside the clip and in 81..127: the first Conv3d
 * (3 input channels) becomes a 1x1 convolution with k_per_tap = 128 */
int qt_pack_clip27(int dtype, const float* clips, void* dst, int batch, int frames, int h, int w, void* stream);
/* One launch per Conv3d block (nn.Conv3d 3x3x3 + BatchNorm3d, /root/reference/3dcnn/models.py:108-139): the operands of
 * the 27-tap implicit GEMM (qt_conv_desc.kt = 3) from nn.Conv3d's weight w [O][I][3][3][3] f32 -- w_fwd
 * [O_pad][27][I_pad], w_dgrad [I_pad][27][O_pad] (optional), zero padded; first != 0: w_fwd [O_pad][128] in the K order of
 * qt_pack_clip27 (27 * I <= 128) -- and the padded per-channel vectors: vec_in_dev = DEVICE array of 5 device pointers
 * (conv bias, BatchNorm weight, bias, running_mean, running_var; [O] each, NULL = padding value) -> vec_out [5][O_pad]
 * padded with 0, 1, 0, 0, 1.  qt_unpack_conv3d_wgrad is the way back for the weight gradient: dw = three [O_pad][9][I_pad]
 * f32 blocks, one per frame tap, as qt_conv2d_wgrad writes them (first != 0: [O_pad][128]) -> grad [O][I][3][3][3]. */
int qt_pack_conv3d_block(int dtype, const float* w, void* w_fwd, void* w_dgrad, int O, int I, int O_pad, int I_pad, int first,
                         const float* const* vec_in_dev, float* vec_out, void* stream);
int qt_unpack_conv3d_wgrad(const float* dw, float* grad, int O, int I, int O_pad, int I_pad, int first, void* stream);
/* BatchNorm3d batch statistics of a finished map y [M][C]: partial[qt_bn_stats_rows(M,C)][2][C] sums / sums of squares
 * (fixed summation order), input of qt_bn_finalize (buffer capacity qt_stats_capacity_rows(rows)) */
int qt_bn_stats_rows(long long M, int C);
int qt_bn_stats(int dtype, const void* y, long long M, int C, float* partial, void* stream);
/* nn.MaxPool3d(kernel = stride = (pool_t, 2, 2)), pool_t 1 or 2, floor mode: x [T][B][H][W][C] ->
 * out [T/pool_t][B][H/2][W/2][C]; argmax (u8 per output element, optional) = index of the first maximum in (t,h,w)
 * scan order, which is where torch's backward sends the gradient.  _bwd writes every element of dx.  C: a positive
 * multiple of 8 (these two and the two fused entry points below; anything else is QT_ERR_INVALID_ARG). */
int qt_pool3d_max(int dtype, const void* x, void* out, unsigned char* argmax, int frames, int batch, int h, int w, int C,
                  int pool_t, void* stream);
int qt_pool3d_max_bwd(int dtype, const void* dout, const unsigned char* argmax, void* dx, int frames, int batch, int h,
                      int w, int C, int pool_t, void* stream);
/* Round 3: BatchNorm3d (scale / shift) + ReLU + MaxPool3d (pool_t, 2, 2) in one pass over the RAW conv output y -- the
 * activation map relu(bn(y)) is not materialised; y_at_max (nullable) keeps y at each pooled cell's argmax, so that the
 * BatchNorm-backward sums can be taken from the pooled side: qt_bn_bwd_reduce(g = d(loss)/d(pooled), mask = pooled,
 * y = y_at_max, M = pooled cells) followed by qt_bn_bwd_finalize with count = ALL positions of the map.  Values compared are
 * the activation rounded to `dtype`, i.e. exactly what qt_bn_act + qt_pool3d_max compare.  y rows are y_channels wide
 * (<= C, a multiple of 8: qt_conv3d_first_fwd writes 32-channel rows while the next layer wants 64-channel K rows);
 * out / argmax / y_at_max rows are C wide and zero in channels >= y_channels. */
int qt_pool3d_bn_relu_max(int dtype, const void* y, const float* scale, const float* shift, void* out, unsigned char* argmax,
                          void* y_at_max, int frames, int batch, int h, int w, int C, int y_channels, int pool_t, void* stream);
/* ... and the backward of the three in one pass: dy = a (g - b - xhat c) with g = dout at the window's argmax where
 * pooled > 0, zero elsewhere (coef = qt_bn_bwd_finalize's [3][C]); replaces qt_pool3d_max_bwd + qt_bn_bwd_apply and the
 * full-size gradient map between them.  dy rows are dy_channels wide (>= y_channels; zero beyond y_channels). */
/* tests: the smallest launch (in 16-byte channel groups) for which qt_pool3d_bn_bwd_apply takes its resident-grid form (bf16, no
 * padding channels: C = y_channels = dy_channels); 0 restores the default (2^20) */
void qt_set_pool3d_apply_light_min(long long groups);
int qt_pool3d_bn_bwd_apply(int dtype, const void* dout, const unsigned char* argmax, const void* pooled, const void* y,
                           const float* mean, const float* invstd, const float* coef, void* dy, int frames, int batch, int h,
                           int w, int C, int y_channels, int dy_channels, int pool_t, void* stream);
/* Round 3: the first Conv3d of the clip models (3 -> 32 channels, 3x3x3, pad 1; /root/reference/3dcnn/models.py:108)
 * straight from the f32 clip [B][T][3][H][W]: y [T][B][H][W][32] (NO channel padding), bias-free accumulator.  w_packed is
 * qt_pack_conv3d_block(first = 1)'s [>= 32][128] filter.  Either scale / shift (+ relu) of 32 channels (eval: folded
 * BatchNorm3d), or stats: qt_conv3d_first_stats_rows(...) rows of [2][64] partial sums of y for qt_bn_finalize (channels
 * 32..63 zero), or neither.  Replaces qt_pack_clip27 + a 1x1 qt_conv2d_igemm over 256-byte K rows (3.3 GB written and read
 * back at 32 x 8 x 224 x 224).  QT_ERR_UNSUPPORTED (take the packed form) for f32, H % 4, W % 16, W > 256, a clip that is
 * not 16-byte aligned, QTCNN_CONV3D_FIRST=0. */
int qt_conv3d_first_stats_rows(int batch, int frames, int h, int w);
/* Round 3: the clip models' second Conv3d (32 -> 64 channels, 3x3x3, pad 1; /root/reference/3dcnn/models.py:115) with the
 * input frame slabs resident in LDS: x [T][B][H][W][x_channels] (channels 0..31 read: the 64-channel-padded pooled map of
 * block 1, or 32-channel rows), w_packed = qt_pack_conv3d_block's [64][27][64], y [T][B][H][W][64].  Bias-free accumulator
 * with either scale / shift (+ relu) of 64 channels, or stats = qt_conv3d_c32_stats_rows(...) rows of [2][64] partial sums
 * for qt_bn_finalize, or neither.  Same result as qt_conv2d_igemm with kt = 3 on the same operands (other summation order).
 * QT_ERR_UNSUPPORTED (take qt_conv2d_igemm) for f32, odd H, W % 16, W > 128, misaligned operands, QTCNN_CONV3D_SLAB=0. */
int qt_conv3d_c32_stats_rows(int batch, int frames, int h, int w);
int qt_conv3d_c32_fwd(int dtype, const void* x, int x_channels, const void* w_packed, void* y, const float* scale,
                      const float* shift, int relu, float* stats, int batch, int frames, int h, int w, void* stream);
/* ... and its data gradient: dx [T][B][H][W][dx_channels] (channels 0..31 = d(loss)/d(input); dx_channels = 64: channels
 * 32..63 written as zeros, the rows a 64-channel-padded conv3d_block1 reads; 32: no padding, round 4) from dy
 * [T][B][H][W][64] and qt_pack_conv3d_block's data-gradient filter [64][27][64] ([input channel][tap][output channel]): the
 * same slab walk over dy with the flipped filter, as two launches over dy's channel halves joined through an f32 scratch
 * (qt_conv3d_c32_dgrad_scratch_bytes; 0 = shape not covered, take qt_conv2d_igemm in QT_CONV_DGRAD mode). */
size_t qt_conv3d_c32_dgrad_scratch_bytes(int batch, int frames, int h, int w);
int qt_conv3d_c32_dgrad(int dtype, const void* dy, const void* w_dgrad_packed, void* dx, int dx_channels, void* scratch,
                        size_t scratch_bytes, int batch, int frames, int h, int w, void* stream);
/* ... and its weight gradient: dweight [64][32][3][3][3] f32 in nn.Conv3d's layout (every element written) from x (channels
 * 0..31 of x_channels-wide rows) and dy [T][B][H][W][64]; the contraction runs over positions with both operands read
 * through transposing LDS reads; per-workgroup partial filters in `workspace` (qt_conv3d_c32_wgrad_workspace_bytes; 0 = shape
 * not covered, take qt_conv2d_wgrad per frame tap) added in a fixed order: deterministic. */
size_t qt_conv3d_c32_wgrad_workspace_bytes(int batch, int frames, int h, int w);
int qt_conv3d_c32_wgrad(int dtype, const void* x, int x_channels, const void* dy, float* dweight, void* workspace,
                        size_t workspace_bytes, int batch, int frames, int h, int w, void* stream);
/* Eval forward of the whole conv3d_block1 in one launch: Conv3d + folded BatchNorm3d (scale / shift of 32 channels, the conv
 * bias folded into shift) + ReLU + MaxPool3d((1,2,2)) in registers; pooled [T][B][H/2][W/2][pooled_channels]: 64 with channels
 * 32..63 zero (the K rows the implicit GEMM reads) or 32 (round 4: what the slab kernels of block 2 read); the conv map never
 * reaches memory.  Same values as qt_conv3d_first_fwd(scale, shift, relu) followed by qt_pool3d_max.  Shapes as
 * qt_conv3d_first_fwd. */
int qt_conv3d_first_fwd_pool(int dtype, const float* clips, const void* w_packed, void* pooled, int pooled_channels,
                             const float* scale, const float* shift, int batch, int frames, int h, int w, void* stream);
/* ... and its weight gradient from the f32 clip and dy [T][B][H][W][32] (32-channel rows, what qt_pool3d_bn_bwd_apply
 * writes with dy_channels = 32): dweight [32][3][3][3][3] f32 in nn.Conv3d's own layout, every element written; partial
 * filters per workgroup in `workspace` (qt_conv3d_first_wgrad_workspace_bytes, 0 = shape not covered: W % 32, else as
 * qt_conv3d_first_fwd) added in a fixed order: deterministic.  Replaces qt_pack_clip27 + qt_conv2d_wgrad +
 * qt_unpack_conv3d_wgrad. */
size_t qt_conv3d_first_wgrad_workspace_bytes(int batch, int frames, int h, int w);
int qt_conv3d_first_wgrad(int dtype, const float* clips, const void* dy, float* dweight, void* workspace,
                          size_t workspace_bytes, int batch, int frames, int h, int w, void* stream);
/* Round 4: the same weight gradient with d(loss)/dy formed on the way in -- the backward of MaxPool3d((1,2,2)) + ReLU +
 * BatchNorm3d of conv3d_block1 (/root/reference/3dcnn/models.py:108-112) inside the weight-gradient kernel: y = the raw conv
 * output [T][B][H][W][32], dout / argmax [T][B][H/2][W/2][pooled_channels] (pooled_channels 32 or 64) = the gradient of the
 * pooled map and qt_pool3d_bn_relu_max's argmax (pool_t = 1), mean / invstd / scale / shift = qt_bn_finalize's vectors,
 * coef = qt_bn_bwd_finalize's [3][pooled_channels].  Replaces qt_pool3d_bn_bwd_apply (dy_channels = 32) +
 * qt_conv3d_first_wgrad: dy (0.8 GB at 32 clips x 8 frames of 224 x 224) is neither written nor read.  The ReLU mask is
 * recomputed from y (relu(y scale + shift) > 0) instead of read from the pooled map.  Workspace and shapes as
 * qt_conv3d_first_wgrad; QT_ERR_UNSUPPORTED otherwise. */
int qt_conv3d_first_wgrad_fused(int dtype, const float* clips, const void* y, const void* dout, const unsigned char* argmax,
                                int pooled_channels, const float* mean, const float* invstd, const float* scale,
                                const float* shift, const float* coef, float* dweight, void* workspace, size_t workspace_bytes,
                                int batch, int frames, int h, int w, void* stream);
int qt_conv3d_first_fwd(int dtype, const float* clips, const void* w_packed, void* y, const float* scale, const float* shift,
                        int relu, float* stats, int batch, int frames, int h, int w, void* stream);
/* ... and its data gradient down to the clip (`image_sequence.grad`): dclips [B][T][3][H][W] f32, the clip's own layout,
 * every element WRITTEN exactly once (no zero fill by the caller, no atomics, the same bits on every run) =
 * conv_transpose3d(dy, w, padding 1) from dy = d(loss)/d(conv output) [T][B][H][W][32] in `dtype` (bf16 or f32; 32-channel
 * rows, what qt_pool3d_bn_bwd_apply writes with dy_channels = 32) and the f32 master filter [32][3][3][3][3] in nn.Conv3d's
 * layout.  bf16 dy in the shapes qt_conv3d_first_fwd takes (H % 4 == 0, W % 16 == 0, W <= 256, 16-byte aligned dy): bf16 MFMA
 * with f32 accumulation, each dy frame slab staged in LDS once for the three frames it reaches; every other shape and f32
 * dy: a direct f32 kernel, one thread per pixel.  bf16 dy is multiplied by the filter rounded to bf16, the rounding
 * qt_pack_conv3d_block applies for the forward.  QT_ERR_UNSUPPORTED only for another dtype. */
int qt_conv3d_first_dgrad(int dtype, const void* dy, const float* w_oidhw, float* dclips, int batch, int frames, int h, int w,
                          void* stream);
/* nn.AdaptiveAvgPool3d((1,1,1)) + flatten(1) into columns [col0, col0+C) of an f32 [B][ld] matrix, and its backward */
int qt_avgpool_tb(int dtype, const void* x, float* dst, int frames, int batch, int hw, int C, int ld, int col0, void* stream);
int qt_avgpool_tb_bwd(int dtype, const float* d, void* g, int frames, int batch, int hw, int C, int ld, int col0,
                      void* stream);

/* ------------------------------------------------------------------------
 * Whole-network executor.  One plan = one model variant at a maximum batch:
 *   QT_MODEL_QUADTREE         QuadtreeCNN  (Quadtree_from scratch/models.py:214-305;
 *                             resnet/models.py:70-180 with `mode`)
 *   QT_MODEL_STANDARD_RESNET  StandardResNetCNN (resnet/models.py:7-65)
 *   QT_MODEL_ATTENTION        AttentionHierarchicalCNN (Quadtree_from scratch/models.py:6-101); `mode` is
 *                             ignored; tensors are listed under base_cnn.* names for the ResNet part (the
 *                             reference keeps it as a local: bind features_extractor.{0,1,4,5} /
 *                             global_processor.{0,1} to base_cnn.{conv1,bn1,layer1,layer2} / {layer3,layer4})
 *   QT_MODEL_CNN_LSTM         CnnLstm (cnn+lstm/models.py:14-89): `batch` counts FRAMES (sequences x seq_len); the
 *                             frozen per-frame ResNet-18 (bind cnn_backbone.{0,1,4,5,6,7} to base_cnn.{conv1,bn1,
 *                             layer1..4}) + Linear-ReLU-Linear on the pose vector feed a 2-layer LSTM over seq_len
 *                             steps; logits [batch / seq_len][num_classes].  Gradients: MLP, LSTM, classifier.
 * The tensor table lists every parameter / buffer under the reference's
 * state_dict key (first-seen `base_cnn.*` names); the caller
 * passes one device pointer per entry (f32, reference layouts: OIHW conv
 * weights, [out][in] linear weights, int64 num_batches_tracked).
 *   qt_plan_pack_weights : casts/permutes the master weights into the packed
 *                          operands (call after every optimizer step)
 *   qt_plan_forward      : model(image[B,3,224,224] f32 NCHW, numerical[B,47] f32)
 *                          -> logits[B,num_classes] f32   (forward of models.py:273-305);
 *                          training == 1: BatchNorm batch statistics + running-stat update, dropout with `seed`;
 *                          training == 0: eval mode, BatchNorm / ReLU / residual fused into the conv epilogues, nothing
 *                          kept for a backbone backward; training == 2: eval-mode arithmetic (running statistics, no
 *                          dropout) but every tensor qt_plan_backward needs is kept, so that model.eval() followed by
 *                          logits.backward() with trainable backbone parameters works (Grad-CAM on the all-trainable
 *                          variant, Quadtree_from scratch/grad_cam.py:72-83)
 *   qt_plan_backward     : loss.backward() of Quadtree_train.py:65 given dlogits;
 *                          grads[i] (f32, same layout as tensors[i]) is written
 *                          (not accumulated) when non-NULL; QT_BWD_HEAD = classifier,
 *                          numerical MLP and quadrant head, QT_BWD_LAYER4 = layer4,
 *                          QT_BWD_LAYER32 = layers 3 and 2, QT_BWD_LAYER1 = layer1 and the stem
 *                          (lets the caller start the gradient all-reduce of a bucket while the
 *                          next phase runs; the last bucket is 0.6 MB).
 *   qt_plan_backward_dx  : the same, and with dimage != NULL also d(loss)/d(image) [B,3,224,224] f32 NCHW (written,
 *                          not accumulated, in the QT_BWD_LAYER1 phase, for the batch of the last forward): the backbone
 *                          is walked for its data gradients even where no backbone gradient is requested (frozen
 *                          backbone: BatchNorm backward and data gradients, no weight gradient), and qt_stem_dgrad
 *                          runs on conv1's output gradient.  Parameter gradients are the same bits as without dimage.
 *                          Needs qt_plan_pack_weights(for_backward = 1) and a forward with training 1 or 2;
 *                          QT_ERR_UNSUPPORTED after training == 0 and for QT_MODEL_CNN_LSTM.  dimage == NULL is
 *                          qt_plan_backward.
 * ------------------------------------------------------------------------ */
enum { QT_MODEL_QUADTREE = 0, QT_MODEL_STANDARD_RESNET = 1, QT_MODEL_ATTENTION = 2, QT_MODEL_CNN_LSTM = 3 };
enum { QT_MODE_FUSION = 0, QT_MODE_IMAGE_ONLY = 1, QT_MODE_NUMERICAL_ONLY = 2 };
/* call order HEAD, LAYER4, LAYER32, LAYER1 (or any union of consecutive phases in one call);
 * QT_BWD_REST = LAYER32 | LAYER1, QT_BWD_BACKBONE = LAYER4 | REST. */
enum { QT_BWD_HEAD = 1, QT_BWD_LAYER4 = 2, QT_BWD_LAYER32 = 4, QT_BWD_LAYER1 = 8, QT_BWD_REST = 12, QT_BWD_BACKBONE = 14,
       QT_BWD_ALL = 15 };

typedef struct qt_plan_desc {
  int dtype;
  int batch;          /* maximum images per call */
  int num_classes;
  int model;
  int mode;
  int numerical_dim;  /* 47 */
  float dropout_p;    /* 0.5 */
  float bn_eps;       /* 1e-5 */
  float bn_momentum;  /* 0.1 */
  int seq_len;        /* QT_MODEL_CNN_LSTM: frames per sequence (reference default 4) */
  int lstm_hidden;    /* QT_MODEL_CNN_LSTM: 256 */
} qt_plan_desc;

typedef struct qt_plan qt_plan;

int qt_plan_create(const qt_plan_desc* desc, qt_plan** out);
void qt_plan_destroy(qt_plan* plan);
int qt_plan_num_tensors(const qt_plan* plan);
const char* qt_plan_tensor_name(const qt_plan* plan, int i);
int qt_plan_tensor_kind(const qt_plan* plan, int i);            /* 0 parameter, 1 f32 buffer, 2 int64 counter */
int qt_plan_tensor_shape(const qt_plan* plan, int i, int* dims4); /* returns ndim */
size_t qt_plan_workspace_bytes(const qt_plan* plan);
/* byte offset inside the workspace of a named activation / gradient buffer:
 * "stem.pooled", "block<0-7>.out|.a1|.gout", "conv<i>.y|.gy", "fused", "dfused", "hidden";
 * QT_MODEL_ATTENTION also "attention.vectors" (f32 [B][16][64]) and "attention.weights" (f32 [B][16]);
 * "conv<i>.dw": the f32 [O][kh][kw][I] slice of the weight-gradient scratch (region "dw") of a convolution whose weight
 * gradient is accumulated there, QT_ERR_INVALID_ARG for one that has none */
int qt_plan_find_buffer(const qt_plan* plan, const char* name, size_t* offset);
/* The workspace layout as a table (tests): every range the plan hands to its launches, in ascending order of offset and
 * disjoint; qt_plan_num_regions is their number. */
int qt_plan_num_regions(const qt_plan* plan);
/* Region i: its name (a short stable string that lives as long as the plan: "stats", "bn7.mean", "conv3.w_dgrad",
 * "block2.a1_bits", "lstm1.gates", "wgrad_part", ...; a buffer qt_plan_find_buffer knows has that name), its byte offset
 * (a multiple of 256) and the bytes asked for it.  The bytes from offset + bytes to the next region's offset (the rounding
 * to 256 and the guard gap) belong to no launch.  The f32 weight-gradient scratch that one memset zeroes per backward is
 * ONE region, "dw", whatever the number of convolutions that own a slice of it. */
int qt_plan_region(const qt_plan* plan, int i, const char** name, size_t* offset, size_t* bytes);
/* Tests: a plan created after this call leaves `bytes` (a multiple of 256, else QT_ERR_INVALID_ARG) unused behind every
 * region of its workspace, qt_plan_workspace_bytes and qt_plan_find_buffer included, so that a launch running over its
 * buffer lands in bytes nobody owns instead of in its neighbour.  Process-wide, read by qt_plan_create; 0 (the default)
 * is the layout without gaps.  Launches, streams and kernel arguments are the same but for the offsets.  The caller's
 * stream workspace of qt_plan_stream_forward (qt_plan_stream_workspace_bytes) is laid out elsewhere and has no gaps. */
int qt_set_plan_guard_gap(size_t bytes);
/* Measurement aid (bench.py roofline): while enabled, every MFMA kernel launch is
 * bracketed by HIP events on its stream; _end sums algorithmic FLOPs, milliseconds
 * and launch counts per kind {0 igemm forward, 1 igemm dgrad, 2 wgrad}. */
int qt_plan_profile_begin(qt_plan* plan);
int qt_plan_profile_end(qt_plan* plan, double* flops3, double* ms3, int* launches3);
/* algorithmic HBM bytes of the launches of the last profile, per kind: every operand of a launch once (source map,
 * weights, destination, per-pixel epilogue operands) -- the figure bench.py puts beside the PMC-measured traffic */
int qt_plan_profile_bytes(const qt_plan* plan, double* bytes3);
/* Weight gradients run on a plan-owned side stream; a partial qt_plan_backward phase returns
 * without joining it.  Before consuming that phase's gradients on another stream (the
 * all-reduce stream), make it wait for the side stream with qt_plan_side_fence (and for the
 * caller's stream as usual).  The last phase joins the side stream into the caller's stream. */
int qt_plan_side_fence(qt_plan* plan, void* waiting_stream);
/* Once per workspace, before the first qt_plan_pack_weights: the constant vectors of the identity BatchNorm affine and the
 * zero tap slots of the merged stride-2 data-gradient operands (qt_pack_dgrad_s2_merged: the packers write the nine real
 * taps only).  Synchronises `stream`. */
int qt_plan_init_workspace(qt_plan* plan, void* workspace, void* stream);
int qt_plan_pack_weights(qt_plan* plan, void* workspace, void* const* tensors, int for_backward, void* stream);
/* Optimizer step fused with the re-packing (replaces optimizer.step() + qt_plan_pack_weights of a
 * training step; Quadtree_from scratch/Quadtree_train.py:66): per plan tensor one gradient pointer
 * (NULL = frozen / unused: only re-packed) and its two Adam moments.  The conv / linear weights are
 * updated inside the one-launch packing kernel, the rest by qt_adam_multi. */
int qt_plan_adam_step(qt_plan* plan, void* workspace, void* const* tensors, float* const* grads, float* const* exp_avg,
                      float* const* exp_avg_sq, const qt_adam_desc* adam, int for_backward, void* stream);
/* qt_plan_adam_step with its bulk beside the fused stem backward.  When the plan's last operation was a full
 * qt_plan_backward (QT_BWD_ALL, no image gradient, bf16, side stream on) whose stem backward ran on `stream`, the batched
 * Adam + re-pack and the plain tensors are enqueued on the plan's side stream, which that backward ordered behind
 * everything it launched before that kernel; conv1's filter (the only gradient the stem backward produces) is updated and packed on `stream`, and `stream`
 * waits for the side stream before the call returns: afterwards the whole step is ordered before later work on
 * `stream`, exactly as for qt_plan_adam_step.  In every other state the call IS qt_plan_adam_step.
 * The side stream is ordered behind the plan's own launches only.  The caller guarantees that nothing enqueued on
 * `stream` since that backward writes the gradients or the optimizer state, or reads or writes the parameters.
 * *overlapped (may be NULL) receives 1 if the overlapped order was used, 0 for the serial one. */
int qt_plan_adam_step_overlapped(qt_plan* plan, void* workspace, void* const* tensors, float* const* grads,
                                 float* const* exp_avg, float* const* exp_avg_sq, const qt_adam_desc* adam, int for_backward,
                                 void* stream, int* overlapped);
/* qt_plan_adam_step with global-norm gradient clipping, all on `stream`: qt_grad_norm_multi over every non-NULL
 * gradient of the plan plus the n_extra gradients of `extra` (tensors outside the plan that share the norm; may be
 * NULL / 0), then the fused step with the gradients scaled by out2[1] as they are read.  The gradients themselves are
 * not written.  `extra` is not updated here: step it with qt_adam_multi_scaled(..., out2 + 1, stream) afterwards.
 * norm_workspace: the size qt_grad_norm_workspace_bytes gives for the same set of gradients (any order).
 * out2: {total_norm, clip_coef} in device memory, as for qt_grad_norm_multi. */
int qt_plan_adam_step_clipped(qt_plan* plan, void* workspace, void* const* tensors, float* const* grads,
                              float* const* exp_avg, float* const* exp_avg_sq, const qt_adam_desc* adam, int for_backward,
                              float max_norm, const qt_adam_item* extra, int n_extra, void* norm_workspace,
                              size_t norm_workspace_bytes, float* out2, void* stream);
int qt_plan_forward(qt_plan* plan, void* workspace, void* const* tensors, const float* image, const float* numerical,
                    float* logits, int batch, int training, unsigned long long seed, void* stream);
/* QT_MODEL_CNN_LSTM on a video stream (the rule: qt_lstm_stream_forward): every frame is embedded once, a window is an
 * addressing rule.  Other models: QT_ERR_UNSUPPORTED with a message.  Eval arithmetic; needs qt_plan_pack_weights.
 *   qt_plan_features       : the per-frame ResNet-18 and the pose MLP for any batch <= the plan's capacity (it need not be a
 *                            multiple of seq_len); stops before the LSTM: buffer "fused" holds the [batch][640] rows.
 *   qt_plan_stream_forward : S streams x n frames, frame-major per stream (image [S*n,3,224,224], numerical [S*n,47],
 *                            S*n <= capacity) -> logits [S*n][num_classes], one row per frame from the window of the last T
 *                            frames (T need not be seq_len).  Features, the f32 cast, layer 0's input product on the route
 *                            of qt_plan_forward, qt_lstm_stream_stage behind carry_in, qt_lstm_stream_forward, the classifier.
 *                            carry_in / carry_out [S][T-1][4H] f32 (two buffers the caller swaps; unused when T == 1;
 *                            rows of carry_in in front of the stream's start never reach a result) and
 *                            stream_workspace (qt_plan_stream_workspace_bytes(plan, S, n, T), 16-byte aligned) are the
 *                            caller's.  No host synchronisation.
 * Both overwrite what qt_plan_backward reads: a backward is refused until the next qt_plan_forward. */
int qt_plan_features(qt_plan* plan, void* workspace, void* const* tensors, const float* image, const float* numerical,
                     int batch, void* stream);
size_t qt_plan_stream_workspace_bytes(const qt_plan* plan, int S, int n, int T);
int qt_plan_stream_forward(qt_plan* plan, void* workspace, void* const* tensors, const float* image, const float* numerical,
                           float* logits, const float* carry_in, float* carry_out, void* stream_workspace,
                           size_t stream_workspace_bytes, long long seen, int S, int n, int T, void* stream);
int qt_plan_backward(qt_plan* plan, void* workspace, void* const* tensors, float* const* grads, const float* numerical,
                     const float* dlogits, int phases, void* stream);
int qt_plan_backward_dx(qt_plan* plan, void* workspace, void* const* tensors, float* const* grads,
                        const float* numerical, const float* dlogits, int phases, float* dimage, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QTCNN_H_ */
