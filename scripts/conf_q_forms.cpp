// Developer aid: the two spellings the integer confidence had before csrc/qt_rowgroup.h's qt_conf_q, compared over every
// one of the 2^32 f32 bit patterns on the host (IEEE fmaxf / fminf / rintf, round to nearest even, as on the device).
//   g++ -O2 -fno-fast-math -o /tmp/conf_q_forms scripts/conf_q_forms.cpp && /tmp/conf_q_forms
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

// timeline.hip's: an explicit NaN test
static int with_test(float x) {
  if (x != x) return 0;
  return (int)rintf(fminf(fmaxf(x, 0.f), 1.f) * 65536.0f);
}
// scores.hip's: fmaxf(NaN, 0) = 0 does the same for a quiet NaN (scores classes a NaN row before it quantises)
static unsigned without_test(float x) { return (unsigned)(int)rintf(fminf(fmaxf(x, 0.f), 1.f) * 65536.0f); }

int main() {
  uint64_t differ = 0, nans = 0, differ_numbers = 0, differ_quiet = 0;
  for (uint64_t b = 0; b < (1ull << 32); ++b) {
    const uint32_t u = (uint32_t)b;
    float x;
    memcpy(&x, &u, 4);
    nans += x != x;
    if ((unsigned)with_test(x) != without_test(x)) {
      ++differ;
      differ_numbers += x == x;
      differ_quiet += x != x && (u & 0x00400000u);   // (the rest are signalling NaNs, which the host's fmaxf hands on)
    }
  }
  printf("%llu patterns, %llu of them NaN; differ: %llu numbers, %llu quiet NaNs, %llu signalling NaNs\n", 1ull << 32,
         (unsigned long long)nans, (unsigned long long)differ_numbers, (unsigned long long)differ_quiet,
         (unsigned long long)(differ - differ_numbers - differ_quiet));
  return differ_numbers != 0 || differ_quiet != 0;
}
