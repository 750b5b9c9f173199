// ld_planes.hpp -- the inner loop ld_band.hip (k_ld_band) and king.hip (k_king) share: two 2-bit records decoded into int8 planes with the
// v_perm table trick of kernels_i8.hip (i8_decode)
//      x = dosage (0 where missing)   table 0x00010002        q = x^2   table 0x00010004        e = 1 - m (missing)   table 0x00000100
// and multiplied on v_mfma_i32_32x32x32_i8 with exact int32 sums.  Device code only; include it from a .hip translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace fpca {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// byte[code] of the three planes, 16 codes of one dword -> 16 bytes each, in the order of i8_decode (codes q, q + 4, q + 8, q + 12 in
// the four bytes of dword q; both operands are decoded alike, so the order within the 32-k step does not matter)
template <bool GENERAL>
__device__ __forceinline__ void ld_decode(uint32_t w, v4i &x, v4i &q, v4i &e)
{
#pragma unroll
   for (int s = 0; s < 4; s++) {
      const uint32_t sel = (w >> (2 * s)) & 0x03030303u;
      x[s] = (int)__builtin_amdgcn_perm(0u, 0x00010002u, sel);
      if (GENERAL) {
         q[s] = (int)__builtin_amdgcn_perm(0u, 0x00010004u, sel);
         e[s] = (int)__builtin_amdgcn_perm(0u, 0x00000100u, sel);
      }
   }
}

// acc[0] += x.x and, GENERAL, acc[1 .. 4] += x.e, e.x, q.e, e.q over `nchunks` chunks of 128 bytes per record; a lane holds the 64 bytes
// of its k-half (pa / pb point at them).  EE: a sixth plane, acc[5] += e.e (the shared-call count of r2; KING's statistic has no use for it)
template <bool GENERAL, bool EE>
__device__ __forceinline__ void ld_products(const uint4 *__restrict__ pa, const uint4 *__restrict__ pb, uint32_t nchunks, v16i (&acc)[EE ? 6 : 5])
{
   uint4 a[4], b[4];
#pragma unroll
   for (int p = 0; p < 4; p++) {
      a[p] = pa[p];
      b[p] = pb[p];
   }
   for (uint32_t c = 0; c < nchunks; c++) {
      // the next chunk's 128 bytes per lane are in flight under this chunk's MFMAs (the last iteration re-reads its own chunk)
      const uint32_t cn = c + 1 < nchunks ? c + 1 : c;
      uint4 an[4], bn[4];
#pragma unroll
      for (int p = 0; p < 4; p++) {
         an[p] = pa[(size_t)cn * 8 + p];
         bn[p] = pb[(size_t)cn * 8 + p];
      }
#pragma unroll
      for (int p = 0; p < 4; p++) {
         const uint32_t wa[4] = {a[p].x, a[p].y, a[p].z, a[p].w}, wb[4] = {b[p].x, b[p].y, b[p].z, b[p].w};
#pragma unroll
         for (int d = 0; d < 4; d++) {
            v4i xa, qa, ea, xb, qb, eb;
            ld_decode<GENERAL>(wa[d], xa, qa, ea);
            ld_decode<GENERAL>(wb[d], xb, qb, eb);
            acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(xa, xb, acc[0], 0, 0, 0);
            if (GENERAL) {
               acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(xa, eb, acc[1], 0, 0, 0);
               acc[2] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ea, xb, acc[2], 0, 0, 0);
               acc[3] = __builtin_amdgcn_mfma_i32_32x32x32_i8(qa, eb, acc[3], 0, 0, 0);
               acc[4] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ea, qb, acc[4], 0, 0, 0);
               if constexpr (EE) acc[5] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ea, eb, acc[5], 0, 0, 0);
            }
         }
      }
#pragma unroll
      for (int p = 0; p < 4; p++) {
         a[p] = an[p];
         b[p] = bn[p];
      }
   }
}

} // namespace fpca
