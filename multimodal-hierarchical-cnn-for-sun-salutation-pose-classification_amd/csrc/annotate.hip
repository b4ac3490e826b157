// Annotated frames on the device (qt_annotate_u8): the pose skeleton of draw_enhanced_skeleton (sqn process/
// processing_image_sequence.py:250-318) and the prediction caption of the video loop (experiment/test_on_video_cnn.py:280-295)
// drawn into a batch of uint8 frames in one launch.  include/qtcnn.h states the rule in full; every test of it is integer.
//
// A workgroup of 256 threads owns AN_TILE = 4096 consecutive pixels of ONE frame (a band of rows, or a piece of one row).
//   1. Threads 0 .. 32 take the frame's landmarks to pixel positions (f32 product, range check, truncation) and leave them in
//      LDS; thread 64 lays out the caption: up to 8 glyph numbers and their pen positions.
//   2. Thread i < n_segments + 33 builds primitive i, in painter's order: segments in list order, then the 33 discs.  A disc
//      is a segment of length 0, so one record serves both: A, d = B - A, L = d.d, R2 (the squared reach of the end caps:
//      floor(T^2 / 4), or r^2), M = floor(sqrt(floor(T^2 L / 4))), the colour, and the bounding box grown by ceil(T / 2)
//      or r.  A primitive can reach a rectangle of pixels when its box meets it and the rectangle does not lie wholly to
//      one side of the stroke (`beside`: four cross products; a long diagonal's box is most of the frame, its stroke is
//      not).  A wave ballot of "can reach the tile" is the tile's list: two 64-bit masks, no compaction, the order is the
//      bit order.
//   3. A thread owns 16 pixels = 48 bytes, laid out as in qt_gradcam_overlay_u8: within a frame the first group starts at
//      the first pixel whose byte address in `out` is a multiple of 16 (3 q + m = 0 mod 16 has the solution q = 5 m mod 16),
//      the fewer than 16 pixels in front of it and behind the last whole group go one per thread with byte accesses, in
//      the frame's first and last workgroup.  The thread keeps the primitives of the tile's list that can reach its own 16
//      pixels (a wave-uniform loop over the list's bits), then walks its sub-list backwards and gives a pixel the colour of
//      the first primitive that covers it: for 16 pixels of one row primitive by primitive, each record read once and e.d,
//      cross and e.x stepped by additions (`paint_row`; measured, EXPERIMENTS.md: per pixel, with the record re-read and a
//      branch per test, the few waves under a dense knot of primitives held the whole launch up); pixel by pixel where the
//      16 wrap into the next row and for heads and tails.  The caption is blended over the result.  A thread that nothing
//      can reach stores what it loaded, and with out == frames it loads and stores nothing; so does a whole tile with an
//      empty list and no caption.
// Narrower arithmetic than the header's 64-bit statement, with the same bits: pixel coordinates are in [0, 8191] and usable
// landmarks in [-8192, 16383], so |e| <= 16383 and |d| <= 24575 per axis: e.e <= 536 805 378, |e.d| and |cross| <=
// 805 224 450 and L <= 1 207 861 250 all fit an int, and every factor fits 24 bits (__mul24, a full-rate instruction where the
// 32-bit multiply is a quarter-rate one); 4 e.e <= T^2 is e.e <= floor(T^2 / 4) because e.e is an integer; cross^2 <= K is
// |cross| <= M = floor(sqrt(K)) for the same reason, and M is taken once per primitive (K <= 225 L / 4 < 2^37 is the only
// 64-bit value), so no pixel pays a 64-bit multiply.
// No atomics, no workspace, no zero fill; a pixel's bytes depend on its own frame's operands only.
#include <math.h>
#include <stdint.h>

#include "qt_common.h"

namespace {

constexpr int AN_THREADS = 256;
constexpr int AN_PIX = 16;                          // pixels per thread: 48 bytes, three 16-byte accesses
constexpr int AN_TILE = AN_THREADS * AN_PIX;        // pixels per workgroup
constexpr int AN_LM = QT_POSE_LANDMARKS;
constexpr int AN_MAX_PRIMS = QT_ANNOTATE_MAX_SEGMENTS + AN_LM;
constexpr int AN_GLYPHS = 8;                        // the class caption + " (d.dd)"; glyphs C .. C+13 are 0-9 . ( ) space
constexpr int AN_MAX_DIM = 8192;
constexpr int AN_MAX_ORIGIN = 1 << 20;
constexpr float AN_COORD_LO = -8192.f, AN_COORD_HI = 16383.f;
static_assert(AN_MAX_PRIMS <= 128, "the tile's list is two wave ballots");

struct AnnArgs {
  const unsigned char* frames;
  unsigned char* out;
  const float4* landmarks;          // or nullptr: no skeleton
  const unsigned char* detected;    // or nullptr
  const unsigned char* segments;
  const long long* pred;            // or nullptr: no caption
  const float* confidence;          // or nullptr
  const unsigned char* atlas;
  const int* widths;
  int H, W, HW, tiles;              // tiles: workgroups per frame
  int n_segments;
  float min_vis;
  int reach2[2], k_t2[2], grow[2];  // segments, [major]: floor(T^2 / 4), T^2, ceil(T / 2)
  int disc_r2[2], disc_r[2];        // discs, [visibility high]
  unsigned line[2], point[2];       // colours [high], byte c in bits 8c .. 8c+7
  unsigned cap_colour;
  int C, gh, gw, ox, oy;
  int src_vec;                      // frames and out agree modulo 16
  int in_place;
};

struct Lists {                      // one workgroup's LDS
  int4 lm[AN_LM];                   // pixel position x, y; usable; visibility high
  int4 box[AN_MAX_PRIMS];           // x0, y0, x1, y1 (inclusive, grown)
  int4 geo[AN_MAX_PRIMS];           // A.x, A.y, d.x, d.y
  int4 par[AN_MAX_PRIMS];           // L, R2, colour, M
  unsigned long long mask[2];       // primitives 0 .. 63 and 64 .. 127 whose box meets the tile
  int pen[AN_GLYPHS + 1];           // glyph k spans columns [pen[k], pen[k + 1])
  int glyph[AN_GLYPHS];
  int n_glyphs;
};

struct Span {                       // inclusive pixel rectangle
  int x0, y0, x1, y1;
};
__device__ __forceinline__ bool meets(const int4& b, const Span& s) {
  return b.x <= s.x1 && b.z >= s.x0 && b.y <= s.y1 && b.w >= s.y0;
}
// the rectangle around pixels p0 .. p1 (inclusive) of a frame W wide; y0 = p0 / W is given
__device__ __forceinline__ Span span_of(int p0, int p1, int y0, int W) {
  Span s;
  s.y0 = y0;
  const int x0 = p0 - y0 * W;
  if (x0 + (p1 - p0) < W) {
    s.y1 = y0;
    s.x0 = x0;
    s.x1 = x0 + (p1 - p0);
  } else {
    s.y1 = p1 / W;
    s.x0 = 0;
    s.x1 = W - 1;
  }
  return s;
}

// floor(sqrt(k)) for 0 <= k < 2^52
__device__ __forceinline__ int isqrt_floor(long long k) {
  long long m = (long long)sqrt((double)k);
  while (m * m > k) --m;
  while ((m + 1) * (m + 1) <= k) ++m;
  return (int)m;
}

// True when the whole rectangle s lies beside the stroke of segment g = (A, d): a covered pixel has |cross| <= M (between the
// ends by the rule; in the round caps because |e x d|^2 <= |e|^2 L <= T^2 L / 4), and cross is affine in the pixel, so over
// s its extremes are at the corners.  (A disc has d = 0: cross is 0 everywhere and this says nothing.)
__device__ __forceinline__ bool beside(const int4& g, int M, const Span& s) {
  const int c00 = __mul24(s.x0 - g.x, g.w) - __mul24(s.y0 - g.y, g.z);
  const int cx = __mul24(s.x1 - s.x0, g.w), cy = __mul24(s.y1 - s.y0, g.z);
  const int c10 = c00 + cx, c01 = c00 - cy, c11 = c10 - cy;
  const int lo = min(min(c00, c10), min(c01, c11)), hi = max(max(c00, c10), max(c01, c11));
  return lo > M || hi < -M;
}

// the bits of m (primitives base .. base + 63) that can reach s
__device__ __forceinline__ unsigned long long cull(unsigned long long m, int base, const Lists& S, const Span& s) {
  unsigned long long keep = 0;
  while (m) {
    const int i = __builtin_ctzll(m);
    m &= m - 1;
    if (meets(S.box[base + i], s) && !beside(S.geo[base + i], S.par[base + i].w, s)) keep |= 1ull << i;
  }
  return keep;
}

__device__ __forceinline__ bool covers(const Lists& S, int i, int x, int y) {
  const int4 g = S.geo[i];
  const int4 p = S.par[i];
  const int ex = x - g.x, ey = y - g.y;
  const int t = __mul24(ex, g.z) + __mul24(ey, g.w);
  if (p.x == 0 || t <= 0) return __mul24(ex, ex) + __mul24(ey, ey) <= p.y;
  if (t >= p.x) {
    const int fx = ex - g.z, fy = ey - g.w;
    return __mul24(fx, fx) + __mul24(fy, fy) <= p.y;
  }
  return abs(__mul24(ex, g.w) - __mul24(ey, g.z)) <= p.w;
}

// the colour of pixel (x, y) under the thread's sub-list: the last primitive that covers it, else `under`
__device__ __forceinline__ unsigned paint(const Lists& S, unsigned long long m0, unsigned long long m1, int x, int y,
                                          unsigned under) {
  while (m1) {
    const int i = 63 - __builtin_clzll(m1);
    m1 &= ~(1ull << i);
    if (covers(S, 64 + i, x, y)) return (unsigned)S.par[64 + i].z;
  }
  while (m0) {
    const int i = 63 - __builtin_clzll(m0);
    m0 &= ~(1ull << i);
    if (covers(S, i, x, y)) return (unsigned)S.par[i].z;
  }
  return under;
}

// The same for 16 pixels of one row, (x .. x + 15, y), primitive by primitive: a primitive's record is read once and e.d,
// cross and e.x step from pixel to pixel by additions (each value is the one `covers` computes for that pixel).  Bit j of the
// result is set where a primitive covers pixel j, and col[j] is then the last such primitive's colour.
__device__ __forceinline__ unsigned paint_row(const Lists& S, unsigned long long m0, unsigned long long m1, int x, int y,
                                              unsigned (&col)[AN_PIX]) {
  unsigned open = (1u << AN_PIX) - 1u;   // pixels no primitive has covered yet
  while ((m0 | m1) != 0 && open != 0) {
    int i;
    if (m1) {
      i = 63 - __builtin_clzll(m1);
      m1 &= ~(1ull << i);
      i += 64;
    } else {
      i = 63 - __builtin_clzll(m0);
      m0 &= ~(1ull << i);
    }
    const int4 g = S.geo[i];
    const int4 p = S.par[i];
    int ex = x - g.x;
    const int ey = y - g.y, fy = ey - g.w;
    const int eyy = __mul24(ey, ey), fyy = __mul24(fy, fy);
    int t = __mul24(ex, g.z) + __mul24(ey, g.w);
    int cross = __mul24(ex, g.w) - __mul24(ey, g.z);
    unsigned hit = 0;
#pragma unroll
    for (int j = 0; j < AN_PIX; ++j) {
      const int fx = ex - g.z;
      const bool h = (p.x == 0 || t <= 0) ? __mul24(ex, ex) + eyy <= p.y
                                          : (t >= p.x ? __mul24(fx, fx) + fyy <= p.y : abs(cross) <= p.w);
      hit |= (h ? 1u : 0u) << j;
      ++ex;
      t += g.z;
      cross += g.w;
    }
    hit &= open;
    open &= ~hit;
#pragma unroll
    for (int j = 0; j < AN_PIX; ++j) col[j] = (hit >> j) & 1u ? (unsigned)p.z : col[j];
  }
  return ~open & ((1u << AN_PIX) - 1u);
}

// the caption blended over colour c of pixel (x, y); called with n_glyphs >= 1
__device__ __forceinline__ unsigned caption(const AnnArgs& a, const Lists& S, int x, int y, unsigned c) {
  const int n = S.n_glyphs;
  if (y < a.oy || y >= a.oy + a.gh || x < S.pen[0] || x >= S.pen[n]) return c;
  int k = 0;
  while (x >= S.pen[k + 1]) ++k;   // ends: x < pen[n]
  const unsigned m = a.atlas[((long long)S.glyph[k] * a.gh + (y - a.oy)) * a.gw + (x - S.pen[k])];
  if (m == 0) return c;
  unsigned r = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const unsigned col = (a.cap_colour >> (8 * ch)) & 0xffu, under = (c >> (8 * ch)) & 0xffu;
    r |= ((m * col + (255u - m) * under + 127u) / 255u) << (8 * ch);
  }
  return r;
}

// bytes 3 J .. 3 J + 2 of twelve little-endian words
template <int J>
__device__ __forceinline__ unsigned get_pixel(const unsigned (&w)[12]) {
  constexpr int i = (3 * J) >> 2, s = 8 * ((3 * J) & 3);
  if constexpr (s <= 8) {
    return (w[i] >> s) & 0xffffffu;
  } else {
    return ((w[i] >> s) | (w[i + 1] << (32 - s))) & 0xffffffu;
  }
}
template <int J>
__device__ __forceinline__ void set_pixel(unsigned (&w)[12], unsigned c) {
  constexpr int i = (3 * J) >> 2, s = 8 * ((3 * J) & 3);
  w[i] = (w[i] & ~(0xffffffu << s)) | (c << s);
  if constexpr (s > 8) w[i + 1] = (w[i + 1] & ~(0xffffffu >> (32 - s))) | (c >> (32 - s));
}

__global__ __launch_bounds__(AN_THREADS) void annotate_kernel(AnnArgs a) {
  __shared__ Lists S;
  const int tid = threadIdx.x;
  const unsigned b = blockIdx.x / (unsigned)a.tiles;
  const int tile = (int)(blockIdx.x - b * (unsigned)a.tiles);
  const long long frame_bytes = 3LL * a.HW * b;
  unsigned char* __restrict__ out = a.out + frame_bytes;
  const unsigned char* __restrict__ src = a.frames + frame_bytes;
  const int W = a.W;

  // this frame's groups and this workgroup's pixels p0 .. p1
  const int m = (int)(reinterpret_cast<uintptr_t>(out) & 15u);
  const int head = min((5 * m) & 15, a.HW);   // first q with 3 q + m = 0 (mod 16)
  const int groups = (a.HW - head) / AN_PIX;
  const int tail = a.HW - head - groups * AN_PIX;
  const bool first = tile == 0, last = tile == a.tiles - 1;
  const int p0 = first ? 0 : head + tile * AN_TILE;
  const int p1 = (last ? a.HW : head + (tile + 1) * AN_TILE) - 1;
  if (p1 < p0) return;
  const Span T = span_of(p0, p1, p0 / W, W);

  // 1. landmarks to pixel positions; the caption's glyphs and pens
  const bool skeleton = a.landmarks != nullptr && (a.detected == nullptr || a.detected[b] != 0);
  if (tid < AN_LM) {
    int4 v = make_int4(0, 0, 0, 0);
    if (skeleton) {
      const float4 l = a.landmarks[(long long)b * AN_LM + tid];
      const float fx = l.x * (float)W, fy = l.y * (float)a.H;
      if (fx >= AN_COORD_LO && fx <= AN_COORD_HI && fy >= AN_COORD_LO && fy <= AN_COORD_HI)   // false for NaN and inf
        v = make_int4((int)fx, (int)fy, 1, l.w > a.min_vis ? 1 : 0);
    }
    S.lm[tid] = v;
  }
  if (tid == 64) {
    int n = 0;
    if (a.pred != nullptr) {
      const long long p = a.pred[b];
      if (p >= 0 && p < (long long)a.C) {
        S.glyph[0] = (int)p;
        n = 1;
        if (a.confidence != nullptr) {
          const float c = a.confidence[b];
          if (c == c) {
            const int v = (int)fminf(fmaxf(rintf(c * 100.0f), 0.f), 100.f);
            S.glyph[1] = a.C + 13;
            S.glyph[2] = a.C + 11;
            S.glyph[3] = a.C + v / 100;
            S.glyph[4] = a.C + 10;
            S.glyph[5] = a.C + v / 10 % 10;
            S.glyph[6] = a.C + v % 10;
            S.glyph[7] = a.C + 12;
            n = AN_GLYPHS;
          }
        }
        int pen = a.ox;
        for (int k = 0; k < n; ++k) {
          int w = a.widths[S.glyph[k]];
          if (w < 0 || w > a.gw) w = 0;
          S.pen[k] = pen;
          pen += w;
        }
        S.pen[n] = pen;
      }
    }
    S.n_glyphs = n;
  }
  __syncthreads();

  // 2. the primitives, and which of them can reach the tile
  if (tid < 128) {
    bool active = false;
    const int n_prims = skeleton ? a.n_segments + AN_LM : 0;
    if (tid < n_prims) {
      int4 A, B;
      bool ok;
      int reach2, grow, t2 = 0;
      unsigned colour;
      if (tid < a.n_segments) {
        const unsigned char* __restrict__ s = a.segments + 3 * tid;
        const unsigned ia = s[0], ib = s[1];
        const int major = s[2] != 0;
        ok = ia < (unsigned)AN_LM && ib < (unsigned)AN_LM;
        A = S.lm[ok ? ia : 0];
        B = S.lm[ok ? ib : 0];
        ok = ok && A.z && B.z;
        reach2 = major ? a.reach2[1] : a.reach2[0];
        grow = major ? a.grow[1] : a.grow[0];
        t2 = major ? a.k_t2[1] : a.k_t2[0];
        colour = (A.w & B.w) ? a.line[1] : a.line[0];
      } else {
        A = B = S.lm[tid - a.n_segments];
        ok = A.z != 0;
        reach2 = A.w ? a.disc_r2[1] : a.disc_r2[0];
        grow = A.w ? a.disc_r[1] : a.disc_r[0];
        colour = A.w ? a.point[1] : a.point[0];
      }
      if (ok) {
        const int dx = B.x - A.x, dy = B.y - A.y;
        const int L = __mul24(dx, dx) + __mul24(dy, dy);
        const int4 box = make_int4(min(A.x, B.x) - grow, min(A.y, B.y) - grow, max(A.x, B.x) + grow, max(A.y, B.y) + grow);
        S.box[tid] = box;
        const int4 geo = make_int4(A.x, A.y, dx, dy);
        const int M = isqrt_floor(((long long)t2 * L) >> 2);   // of K = floor(T^2 L / 4), both factors >= 0
        S.geo[tid] = geo;
        S.par[tid] = make_int4(L, reach2, (int)colour, M);
        active = meets(box, T) && !beside(geo, M, T);
      }
    }
    const unsigned long long bal = __ballot(active);
    if ((tid & 63) == 0) S.mask[tid >> 6] = bal;
  }
  __syncthreads();

  // 3. the pixels
  const unsigned long long tm0 = S.mask[0], tm1 = S.mask[1];
  const int n_glyphs = S.n_glyphs;
  Span cap;   // the caption's rectangle
  cap.x0 = n_glyphs ? S.pen[0] : 0;
  cap.x1 = n_glyphs ? S.pen[n_glyphs] - 1 : -1;
  cap.y0 = a.oy;
  cap.y1 = a.oy + a.gh - 1;
  const bool tile_cap = cap.x1 >= cap.x0 && meets(make_int4(cap.x0, cap.y0, cap.x1, cap.y1), T);
  if (!(tm0 | tm1) && !tile_cap && a.in_place) return;

  const int g = tile * AN_THREADS + tid;
  if (g < groups) {
    const int q0 = head + g * AN_PIX;
    int y = q0 / W, x = q0 - y * W;
    const Span R = span_of(q0, q0 + AN_PIX - 1, y, W);
    const unsigned long long m0 = cull(tm0, 0, S, R), m1 = cull(tm1, 64, S, R);
    const bool my_cap = tile_cap && meets(make_int4(cap.x0, cap.y0, cap.x1, cap.y1), R);
    const bool touched = (m0 | m1) != 0 || my_cap;
    if (touched || !a.in_place) {
      unsigned w[12];
      if (a.src_vec) {
        const uint4* __restrict__ s = reinterpret_cast<const uint4*>(src + 3LL * q0);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const uint4 u = s[k];
          w[4 * k] = u.x; w[4 * k + 1] = u.y; w[4 * k + 2] = u.z; w[4 * k + 3] = u.w;
        }
      } else {
        const unsigned char* __restrict__ s = src + 3LL * q0;
#pragma unroll
        for (int k = 0; k < 12; ++k)
          w[k] = (unsigned)s[4 * k] | ((unsigned)s[4 * k + 1] << 8) | ((unsigned)s[4 * k + 2] << 16) |
                 ((unsigned)s[4 * k + 3] << 24);
      }
      if (touched && R.y0 == R.y1) {   // the 16 pixels are in one row: primitive by primitive
        unsigned col[AN_PIX] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        const unsigned covered = paint_row(S, m0, m1, x, y, col);
        static_for<AN_PIX>([&](auto j) {
          constexpr int J = decltype(j)::value;
          const unsigned under = get_pixel<J>(w);
          unsigned c = (covered >> J) & 1u ? col[J] : under;
          if (my_cap) c = caption(a, S, x + J, y, c);
          if (c != under) set_pixel<J>(w, c);
        });
      } else if (touched) {            // they wrap into the next row: pixel by pixel
        static_for<AN_PIX>([&](auto j) {
          const unsigned under = get_pixel<decltype(j)::value>(w);
          unsigned c = paint(S, m0, m1, x, y, under);
          if (my_cap) c = caption(a, S, x, y, c);
          if (c != under) set_pixel<decltype(j)::value>(w, c);
          if (++x == W) {
            x = 0;
            ++y;
          }
        });
      }
      uint4* __restrict__ d = reinterpret_cast<uint4*>(out + 3LL * q0);
      d[0] = make_uint4(w[0], w[1], w[2], w[3]);
      d[1] = make_uint4(w[4], w[5], w[6], w[7]);
      d[2] = make_uint4(w[8], w[9], w[10], w[11]);
    }
  }
  // the pixels in front of the frame's first group (its first workgroup) and behind its last one (its last workgroup)
  auto one_pixel = [&](int q) {
    const int y = q / W, x = q - y * W;
    const Span R = {x, y, x, y};
    const unsigned long long m0 = cull(tm0, 0, S, R), m1 = cull(tm1, 64, S, R);
    const bool my_cap = tile_cap && meets(make_int4(cap.x0, cap.y0, cap.x1, cap.y1), R);
    const bool touched = (m0 | m1) != 0 || my_cap;
    if (!touched && a.in_place) return;
    const unsigned char* __restrict__ s = src + 3LL * q;
    const unsigned under = (unsigned)s[0] | ((unsigned)s[1] << 8) | ((unsigned)s[2] << 16);
    unsigned c = under;
    if (touched) {
      c = paint(S, m0, m1, x, y, under);
      if (my_cap) c = caption(a, S, x, y, c);
    }
    unsigned char* __restrict__ d = out + 3LL * q;
    d[0] = (unsigned char)(c & 0xffu);
    d[1] = (unsigned char)((c >> 8) & 0xffu);
    d[2] = (unsigned char)((c >> 16) & 0xffu);
  };
  if (first && tid < head) one_pixel(tid);
  if (last && tid < tail) one_pixel(head + groups * AN_PIX + tid);
}

unsigned pack3(const unsigned char (&c)[3]) { return (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16); }
bool in_1_15(int v) { return v >= 1 && v <= 15; }
uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

}  // namespace

extern "C" int qt_annotate_u8(const qt_annotate_desc* desc, const unsigned char* frames, const float* landmarks,
                              const unsigned char* detected, const unsigned char* segments, const long long* pred,
                              const float* confidence, const unsigned char* atlas, const int* atlas_widths,
                              unsigned char* out, void* stream) {
  QT_CHECK_ARG(desc != nullptr, "qt_annotate_u8: null descriptor");
  const qt_annotate_desc& d = *desc;
  QT_CHECK_ARG(d.batch >= 1 && d.H >= 1 && d.W >= 1, "qt_annotate_u8: sizes must be positive (batch %d, frames %d x %d)", d.batch,
               d.H, d.W);
  QT_CHECK_ARG(frames != nullptr && out != nullptr, "qt_annotate_u8: null frames / output");
  const bool skeleton = landmarks != nullptr, text = pred != nullptr;
  QT_CHECK_ARG((landmarks != nullptr) == (segments != nullptr) && (detected == nullptr || skeleton),
               "qt_annotate_u8: the skeleton group is landmarks and segments together (detected only with them)");
  QT_CHECK_ARG((pred != nullptr) == (atlas != nullptr) && (pred != nullptr) == (atlas_widths != nullptr) &&
                   (confidence == nullptr || text),
               "qt_annotate_u8: the caption group is pred, atlas and atlas_widths together (confidence only with them)");
  QT_CHECK_ARG(skeleton || text, "qt_annotate_u8: nothing to draw: neither the skeleton group nor the caption group is given");
  QT_CHECK_ARG((addr(landmarks) & 15) == 0, "qt_annotate_u8: landmarks must be 16-byte aligned");
  QT_CHECK_ARG((addr(pred) & 7) == 0 && ((addr(confidence) | addr(atlas_widths)) & 3) == 0,
               "qt_annotate_u8: pred must be 8-byte aligned, confidence and atlas_widths 4-byte aligned");
  if (skeleton) {
    QT_CHECK_ARG(d.n_segments >= 0 && d.n_segments <= QT_ANNOTATE_MAX_SEGMENTS,
                 "qt_annotate_u8: n_segments must be in [0, %d] (got %d)", QT_ANNOTATE_MAX_SEGMENTS, d.n_segments);
    QT_CHECK_ARG(in_1_15(d.thick_major) && in_1_15(d.thick_minor) && in_1_15(d.radius_hi) && in_1_15(d.radius_lo),
                 "qt_annotate_u8: thickness and radius must be in [1, 15] (got thickness %d / %d, radius %d / %d)", d.thick_major,
                 d.thick_minor, d.radius_hi, d.radius_lo);
    QT_CHECK_ARG(d.min_visibility == d.min_visibility, "qt_annotate_u8: min_visibility is NaN");
  }
  if (text)
    QT_CHECK_ARG(d.num_classes >= 1 && d.glyph_h >= 1 && d.glyph_w >= 1,
                 "qt_annotate_u8: a caption needs num_classes, glyph_h and glyph_w >= 1 (got %d, %d, %d)", d.num_classes, d.glyph_h,
                 d.glyph_w);
  const long long bytes = 3LL * d.batch * d.H * d.W;   // < 2^63: three ints
  if (d.H > AN_MAX_DIM || d.W > AN_MAX_DIM || bytes > (1LL << 31)) {
    qt_set_error("qt_annotate_u8: %d frames of %d x %d: at most %d lines or columns and 2^31 bytes are handled", d.batch, d.H, d.W,
                 AN_MAX_DIM);
    return QT_ERR_UNSUPPORTED;
  }
  if (text && (d.glyph_h > AN_MAX_DIM || d.glyph_w > AN_MAX_DIM || d.ox > AN_MAX_ORIGIN || d.ox < -AN_MAX_ORIGIN ||
               d.oy > AN_MAX_ORIGIN || d.oy < -AN_MAX_ORIGIN)) {
    qt_set_error("qt_annotate_u8: glyphs of %d x %d at (%d, %d): at most %d lines or columns and an origin within +-%d are handled",
                 d.glyph_h, d.glyph_w, d.ox, d.oy, AN_MAX_DIM, AN_MAX_ORIGIN);
    return QT_ERR_UNSUPPORTED;
  }
  QT_CHECK_ARG(out == frames || addr(out) + (uintptr_t)bytes <= addr(frames) || addr(frames) + (uintptr_t)bytes <= addr(out),
               "qt_annotate_u8: out overlaps frames without being frames itself");
  AnnArgs a;
  a.frames = frames;
  a.out = out;
  a.landmarks = reinterpret_cast<const float4*>(landmarks);
  a.detected = detected;
  a.segments = segments;
  a.pred = pred;
  a.confidence = confidence;
  a.atlas = atlas;
  a.widths = atlas_widths;
  a.H = d.H;
  a.W = d.W;
  a.HW = d.H * d.W;
  a.tiles = max(1, qt_cdiv(a.HW / AN_PIX, AN_THREADS));   // a frame has at most HW / 16 whole groups at any alignment
  a.n_segments = skeleton ? d.n_segments : 0;
  a.min_vis = d.min_visibility;
  const int thick[2] = {d.thick_minor, d.thick_major}, radius[2] = {d.radius_lo, d.radius_hi};
  for (int k = 0; k < 2; ++k) {
    a.k_t2[k] = thick[k] * thick[k];
    a.reach2[k] = a.k_t2[k] / 4;
    a.grow[k] = (thick[k] + 1) / 2;
    a.disc_r2[k] = radius[k] * radius[k];
    a.disc_r[k] = radius[k];
  }
  a.line[0] = pack3(d.line_lo);
  a.line[1] = pack3(d.line_hi);
  a.point[0] = pack3(d.point_lo);
  a.point[1] = pack3(d.point_hi);
  a.cap_colour = pack3(d.caption_colour);
  a.C = d.num_classes;
  a.gh = text ? d.glyph_h : 1;
  a.gw = text ? d.glyph_w : 1;
  a.ox = d.ox;
  a.oy = d.oy;
  a.src_vec = ((addr(frames) ^ addr(out)) & 15u) == 0;
  a.in_place = out == frames;
  const long long blocks = (long long)d.batch * a.tiles;   // <= 2^31 / 3 frames + 2^31 / (48 * 256) tiles
  hipLaunchKernelGGL(annotate_kernel, dim3((unsigned)blocks), dim3(AN_THREADS), 0, static_cast<hipStream_t>(stream), a);
  QT_CHECK_LAUNCH();
  return QT_OK;
}
