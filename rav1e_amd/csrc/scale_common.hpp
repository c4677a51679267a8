// scale_common.hpp -- DistortionScale's fixed-point arithmetic and the binary log / exp it rests on, each rule
// stated once for the device kernels and the host function of scales.hip:
//   ds_new         DistortionScale::new (rdo.rs:578-583): rounded quotient in Q14, saturated to 2^28 - 1
//   ds_from_f64    From<f64> (rdo.rs:652-658)
//   ds_mul         Mul (rdo.rs:618-630): round, shift 14, clamp to [1, 2^28 - 1]
//   blog32_q11     util/logexp.rs:271-286      bexp64  :34-125      blog64  :130-174
// (DistortionScale::mul_u64 and the lookup of a block's scale are dist_common.hpp's: they serve the distortions.)
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace r1scale {

constexpr int DS_SHIFT = 14;
constexpr uint64_t DS_MAX = (1ull << 28) - 1;

__host__ __device__ inline uint32_t ds_new(uint64_t num, uint64_t den) {
  // `num << SHIFT` drops what it shifts out, as Rust's << does; the addition saturates
  const uint64_t sh = num << DS_SHIFT, half = den / 2;
  const uint64_t sum = sh > ~0ull - half ? ~0ull : sh + half;
  const uint64_t raw = sum / den;
  return (uint32_t)(raw <= DS_MAX ? raw : DS_MAX);
}

// `scale * 2^15 as u64` is Rust's saturating float cast: NaN and negatives 0, 2^64 and above u64::MAX
__host__ __device__ inline uint32_t ds_from_f64(double scale) {
  const double v = scale * 32768.0;
  uint64_t num;
  if (!(v > 0.0)) num = 0;
  else if (v >= 18446744073709551616.0) num = ~0ull;
  else num = (uint64_t)v;
  return ds_new(num, 32768);
}

__host__ __device__ inline uint32_t ds_mul(uint32_t a, uint32_t b) {
  const uint64_t v = ((uint64_t)a * b + (1u << (DS_SHIFT - 1))) >> DS_SHIFT;
  return (uint32_t)(v < 1 ? 1 : v > DS_MAX ? DS_MAX : v);
}

// Q0 in, Q11 out: a quartic on the mantissa (i32 arithmetic, no product leaves 32 bits)
__host__ __device__ inline int32_t blog32_q11(uint32_t w) {
  if (w == 0) return -1;
  const int ipart = 32 - __builtin_clz(w);
  const int32_t n = (int32_t)(ipart - 16 > 0 ? w >> (ipart - 16) : w << (16 - ipart)) - 32768 - 16384;
  const int32_t fpart =
      ((n * (((n * (((n * (((n * -1402) >> 15) + 2546)) >> 15) - 5216)) >> 15) + 15745)) >> 15) - 6797;
  return (ipart << 11) + (fpart >> 3);
}

__host__ __device__ inline int64_t atanh_log2(int i) {
  constexpr int64_t T[32] = {
      0x32B803473F7AD0F4, 0x2F2A71BD4E25E916, 0x2E68B244BB93BA06, 0x2E39FB9198CE62E4, 0x2E2E683F68565C8F,
      0x2E2B850BE2077FC1, 0x2E2ACC58FE7B78DB, 0x2E2A9E2DE52FD5F2, 0x2E2A92A338D53EEC, 0x2E2A8FC08F5E19B6,
      0x2E2A8F07E51A485E, 0x2E2A8ED9BA8AF388, 0x2E2A8ECE2FE7384A, 0x2E2A8ECB4D3E4B1A, 0x2E2A8ECA94940FE8,
      0x2E2A8ECA6669811D, 0x2E2A8ECA5ADEDD6A, 0x2E2A8ECA57FC347E, 0x2E2A8ECA57438A43, 0x2E2A8ECA57155FB4,
      0x2E2A8ECA5709D510, 0x2E2A8ECA5706F267, 0x2E2A8ECA570639BD, 0x2E2A8ECA57060B92, 0x2E2A8ECA57060008,
      0x2E2A8ECA5705FD25, 0x2E2A8ECA5705FC6C, 0x2E2A8ECA5705FC3E, 0x2E2A8ECA5705FC33, 0x2E2A8ECA5705FC30,
      0x2E2A8ECA5705FC2F, 0x2E2A8ECA5705FC2F};
  return T[i];
}

__host__ __device__ inline int64_t q57(int v) { return (int64_t)v * ((int64_t)1 << 57); }

// 2^(logq57 / 2^57) by hyperbolic CORDIC; iterations 4, 13 and 40 run twice, as the reference has them
__host__ __device__ inline int64_t bexp64(int64_t logq57) {
  const int ipart = (int)(logq57 >> 57);
  if (ipart < 0) return 0;
  if (ipart >= 63) return 0x7FFFFFFFFFFFFFFF;
  int64_t z = logq57 - q57(ipart), w;
  if (z != 0) {
    z *= 32;
    w = 0x26A3D0E401DD846D;
    int i = 0;
    for (;;) {
      const int64_t mask = -(int64_t)(z < 0);
      w += ((w >> (i + 1)) + mask) ^ mask;
      z -= (atanh_log2(i) + mask) ^ mask;
      if (i >= 3) break;   // repeat iteration 4
      z *= 2;
      i++;
    }
    for (;;) {
      const int64_t mask = -(int64_t)(z < 0);
      w += ((w >> (i + 1)) + mask) ^ mask;
      z -= (atanh_log2(i) + mask) ^ mask;
      if (i >= 12) break;  // repeat iteration 13
      z *= 2;
      i++;
    }
    for (; i < 32; i++) {
      const int64_t mask = -(int64_t)(z < 0);
      w += ((w >> (i + 1)) + mask) ^ mask;
      z = (z - ((atanh_log2(i) + mask) ^ mask)) * 2;
    }
    uint32_t wlo = 0;      // the reference's i32, kept unsigned here: its additions may wrap
    if (ipart > 30) {
      for (;;) {
        const int64_t mask = -(int64_t)(z < 0);
        wlo += (uint32_t)(((w >> i) + mask) ^ mask);
        z -= (atanh_log2(31) + mask) ^ mask;
        if (i >= 39) break;  // repeat iteration 40
        z *= 2;
        i++;
      }
      for (; i < 61; i++) {
        const int64_t mask = -(int64_t)(z < 0);
        wlo += (uint32_t)(((w >> i) + mask) ^ mask);
        z = (z - ((atanh_log2(31) + mask) ^ mask)) * 2;
      }
    }
    w = (w << 1) + (int64_t)(int32_t)wlo;
  } else {
    w = (int64_t)1 << 62;
  }
  if (ipart < 62) w = ((w >> (61 - ipart)) + 1) >> 1;
  return w;
}

// log2(n) in Q57, the inverse rotation; the same repeated iterations
__host__ __device__ inline int64_t blog64(int64_t n) {
  if (n <= 0) return -1;
  const int ipart = 63 - __builtin_clzll((unsigned long long)n);
  const int64_t w = ipart > 61 ? n >> (ipart - 61) : n << (61 - ipart);
  if ((w & (w - 1)) == 0) return q57(ipart);
  int64_t z = 0;
  int64_t x = w + ((int64_t)1 << 61), y = w - ((int64_t)1 << 61);
  const int bounds[4] = {3, 12, 39, 61};
  int i = 0;
  for (int j = 0; j < 4; j++) {
    for (;;) {
      const int64_t mask = -(int64_t)(y < 0);
      z += ((atanh_log2(i < 31 ? i : 31) >> i) + mask) ^ mask;
      const int64_t u = x >> (i + 1);
      x -= ((y >> (i + 1)) + mask) ^ mask;
      y -= (u + mask) ^ mask;
      if (i == bounds[j]) break;
      i++;
    }
  }
  z = (z + 8) >> 4;
  return q57(ipart) + z;
}

}  // namespace r1scale
