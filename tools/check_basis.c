/* Verification of basis1() in dazimsurftomo_amd/csrc/rays.hip: the per-lane form of one cubic B-spline basis element,
 *   w = (i == 0 ? 1 - v : v), t2 = w * w, t3 = t2 * w, p = (i == 1 ? 4 : 1 + 3 v), (c, d) = (i == 1 ? (-6, 3) : (3, -3)),
 *   element = divr((i == 0 || i == 3) ? t3 : (p + c * t2) + d * t3, 1 / 6),
 * equals the plain form that computes the four numerators of inv/CalSurfG.f90:2145-2148 and selects one, for i = 0..3 and EVERY
 * float v (all 2^32 bit patterns; numerator and element compared bit for bit, the sign of a zero included; NaN results compared
 * as NaN: the payload a NaN carries through an addition is the processor's choice, not the formula's).
 *   gcc -O2 -ffp-contract=off -o check_basis tools/check_basis.c -lm
 *   ./check_basis [stride]      stride 1 = exhaustive (~3 min); zeros, denormals, infinities and NaNs are always included;
 *                               prints the mismatch count */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
static float div6(float x) { return (float)((double)x * (1.0 / 6.0)); }
static float plain_num(float v, int i) {
  const float om = 1.0f - v;
  const float n0 = om * om * om;
  const float n1 = 4.0f - 6.0f * (v * v) + 3.0f * (v * v * v);
  const float n2 = 1.0f + 3.0f * v + 3.0f * (v * v) - 3.0f * (v * v * v);
  const float n3 = v * v * v;
  return i == 0 ? n0 : (i == 1 ? n1 : (i == 2 ? n2 : n3));
}
static float lane_num(float v, int i) {
  const float w = i == 0 ? 1.0f - v : v;
  const float t2 = w * w, t3 = t2 * w;
  const float p = i == 1 ? 4.0f : 1.0f + 3.0f * v;
  const float c = i == 1 ? -6.0f : 3.0f, d = i == 1 ? 3.0f : -3.0f;
  const float n = (p + c * t2) + d * t3;
  return (i == 0 || i == 3) ? t3 : n;
}
static int same(float a, float b) {
  uint32_t x, y;
  if (isnan(a) && isnan(b)) return 1;
  memcpy(&x, &a, 4);
  memcpy(&y, &b, 4);
  return x == y;
}
static uint64_t check(uint32_t bits) {
  /* volatile: the index reaches both forms as a run-time value, as the lane's index does in the kernel */
  static volatile int idx[4] = {0, 1, 2, 3};
  uint64_t bad = 0;
  float v;
  memcpy(&v, &bits, 4);
  for (int k = 0; k < 4; k++) {
    const int i = idx[k];
    const float a = plain_num(v, i), b = lane_num(v, i);
    if (!same(a, b) || !same(div6(a), div6(b))) bad++;
  }
  return bad;
}
int main(int argc, char **argv) {
  const uint64_t stride = argc > 1 ? (uint64_t)atoll(argv[1]) : 1;
  static const uint32_t special[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu, 0x00800000u,
                                     0x80800000u, 0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u,
                                     0x7f800001u, 0xff800001u, 0x7fffffffu, 0xffffffffu, 0x3f800000u, 0xbf800000u, 0x3f000000u,
                                     0x3f7fffffu, 0x3f800001u, 0x33800000u, 0x34000000u};
  uint64_t bad = 0, n = 0;
  if (stride == 0) return 2;
  for (unsigned s = 0; s < sizeof special / sizeof special[0]; s++, n++) bad += check(special[s]);
  for (uint64_t b = 0; b <= 0xffffffffull; b += stride, n++) bad += check((uint32_t)b);
  printf("basis1, i = 0..3: %llu mismatches of %llu values\n", (unsigned long long)bad, (unsigned long long)n);
  return bad != 0;
}
