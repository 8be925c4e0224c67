// AdaptiveAvgPool2d(7) bin arithmetic and the backward's per-pixel gather, shared by the pool kernels
// (attention.hip) and the LayerNorm backward that folds the depth branch's pooled-query gradient into its
// dy load (layernorm.hip): one source for both, so the two produce the same bits.
#pragma once
#include "common.h"

DFM_INLINE int bin_lo(int i, int n) { return (i * n) / 7; }
DFM_INLINE int bin_hi(int i, int n) { return ((i + 1) * n + 6) / 7; }

// s[0..V) = sum over the bins pixel (h, w) of image b lies in, i then j ascending, of
// dy[b * 49 + i * 7 + j][c .. c + V) * (1 / bin size), each term one fma onto s (V = 8, or 4 for fp32 rows
// moved as 16-byte vectors).
template <typename T, int V>
DFM_INLINE void pool7_gather(const T* __restrict__ dy, long lddy, int b, int h, int w, int H, int W, int c, float* s) {
#pragma unroll
  for (int q = 0; q < V; ++q) s[q] = 0.f;
  // for n >= 7 a row lies in bins ic-1..ic+1 only; smaller maps repeat rows over more bins
  const int ic = (h * 7) / H, jc = (w * 7) / W;
  const int ia = H >= 7 ? max(0, ic - 1) : 0, ib = H >= 7 ? min(6, ic + 1) : 6;
  const int ja = W >= 7 ? max(0, jc - 1) : 0, jb = W >= 7 ? min(6, jc + 1) : 6;
  for (int i = ia; i <= ib; ++i) {
    const int ha = bin_lo(i, H), hb = bin_hi(i, H);
    if (h < ha || h >= hb) continue;
    for (int j = ja; j <= jb; ++j) {
      const int wa = bin_lo(j, W), wb = bin_hi(j, W);
      if (w < wa || w >= wb) continue;
      const float inv = 1.f / (float)((hb - ha) * (wb - wa));
      float v[V];
      const T* p = dy + ((long)b * 49 + i * 7 + j) * lddy + c;
      if constexpr (V == 8) {
        ld8<T>(p, v);
      } else {
        static_assert(V == 4 && sizeof(T) == 4, "4-element vectors are fp32 rows");
        const float4 f = *reinterpret_cast<const float4*>(p);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
      }
#pragma unroll
      for (int q = 0; q < V; ++q) s[q] = fmaf(v[q], inv, s[q]);
    }
  }
}
