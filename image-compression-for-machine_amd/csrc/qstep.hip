// Quantiser step on the latent y (the codec's quality knob), gfx950.  Parity unpinned: no counterpart in the reference.
//
// With a step D = 2^(k/8) the codec codes round((y - mu) / D) under the predicted Gaussian of scale sigma / D and
// rebuilds y_hat = s D + mu.  The host passes two floats, `step` = D and `inv` = 1 / D, both derived from k in one
// place (icm_amd/bitstream.py: step_of); the arithmetic below is all f32, every operation rounded once:
//
//     t = y - mu;  u = t * inv;  s = rint(u) clamped to +-2^30;  symbol = (int)s
//     y_hat = ((float)symbol * step) + mu            a multiply, then an add: never an FMA
//     se = max(scale, scale_bound) * inv
//     index = (ns - 1) - #{ j < ns - 1 : se <= table[j] }       the count of gc_build_indexes_kernel (entropy.hip)
//
// The decoder has the integer symbol, mu and scale, and must arrive at the encoder's y_hat and index bit for bit, and
// the trainer at the codec's y_hat: every expression has ONE statement here, an element function that each kernel
// calls with the (step, inv) pair of its element, and the kernels differ only in where that pair comes from and in how
// they walk the grid.  `symbol_of`, `yh_of` and `index_of` are the three expressions, `code_elem` / `code_store` the
// encoder's element, `lik_fwd_elem` / `lik_bwd_elem` the training step's.  (y_hat is formed from the symbol after its
// trip through int, in the encoder too, so a -0 of rint is the +0 the decoder sees.)  With step = inv = 1 the symbols
// are icm_quantize's, the indexes icm_gc_build_indexes' and y_hat the fused forward's.
//
// The pair comes from one of three places:
//   scalar     two kernel arguments, one pair for the whole launch                     (_q kernels)
//   per image  `steps` [N] float2 in device memory (a captured training graph is replayed with fresh steps); the pair of
//              image n is a wave-uniform 8-byte load per element, N pairs that stay in cache       (_qs kernels)
//   map        `qmap` int8 step indexes k per latent position, shared by the channels, and `steps`, 256 (step, inv)
//              pairs indexed by the map byte read as unsigned (icm_amd/bitstream.py: step_table; bytes that are no valid
//              k hold (1, 1), so no byte indexes outside it and nothing here clamps or branches on validity).  The
//              codec's map is [HW], shared by every n; the trainer's [N][HW].      (_qmap, _qm kernels; _rdo takes either)
//
// All of it is memory-bound elementwise work on [N][C][HW] operands that are channel slices of wider buffers (an element
// batch stride per float operand; the int32 outputs are dense), one element per lane and pass, consecutive lanes on
// consecutive addresses in every operand.  The table index j of index_of is wave-uniform, so the 64-entry table is read
// through the scalar cache, also where `se` differs per lane; no LDS.  The grid is walked in one of three ways, each
// loop spelled out in its kernels (a shared traversal taking the element as a callable changed the flat kernels'
// instruction streams; the bodies are what must agree):
//   flat       a grid-stride loop over i = n per + r.  The codec's grid is capped at one 256-thread workgroup per CU
//              (q_blocks), which covers the slice of the largest image one compress() call takes, under a million
//              elements, in a few passes (measured: 19 us for the fused kernel on the 786 432 elements of a 2048x3072
//              image's slice, against 45 us for the three launches it replaces).
//   map        a 3-D grid, x over HW, y over c, z over n, each a grid-stride loop (qmap_grid), so a position index is
//              never divided out of a flat one.  A lane reads its map byte and its pair once per position (consecutive
//              lanes on consecutive map bytes: 64 bytes per wave) and keeps them in registers over the channels and
//              images it walks.  The pairs are read with plain global loads (one 8-byte load per lane and position; the
//              table is 2 KB, read-only and stays in cache); the plain form is the one kept and an LDS-staged table was
//              not needed: on the 786 432-element slice the fused map kernel measured 19.9 - 20.0 us against the scalar
//              kernel's 19.5 - 19.9 us in the same run.
//   map, z = n the same with z the image itself (qm_grid): a training or codec batch is small, and with n fixed per
//              workgroup the operand offsets n * bs fold into the base pointers once (with a loop over n the backward
//              kernel ran out of scalar registers and the RDOQ kernel spilled them).
#include <algorithm>
#include <cmath>
#include <initializer_list>
#include "icm_common.h"
#include "image_u8.h"

namespace icm {

// One rounding each, never fused (the reasoning is at the same pair in imageio.hip: under contract(off) the operators
// stay a v_mul / v_add pair, where __fmul_rn / __fadd_rn get folded into an FMA).
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

constexpr float SYMBOL_MAX = 1073741824.0f;   // 2^30: the cast to int is defined for every finite input

__device__ __forceinline__ int symbol_of(float y, float mu, float inv) {
  const float s = rintf(mul_rn(y - mu, inv));   // half to even
  return (int)fminf(fmaxf(s, -SYMBOL_MAX), SYMBOL_MAX);
}
__device__ __forceinline__ float yh_of(int symbol, float mu, float step) {
  return add_rn(mul_rn((float)symbol, step), mu);
}
__device__ __forceinline__ int index_of(float scale, float bound, float inv, const float* __restrict__ table, int ns) {
  const float se = mul_rn(fmaxf(scale, bound), inv);
  int v = ns - 1;
#pragma unroll 8   // j is wave-uniform: eight entries per scalar load and wait
  for (int j = 0; j < ns - 1; ++j) v -= (se <= table[j]) ? 1 : 0;
  return v;
}

// shape and batch strides (elements) of the operands; a stride of an operand a kernel does not take is unused
struct QGeom {
  long long y_bs, mu_bs, sc_bs, yh_bs;
  int N, C, HW;
};

// ---- the encoder's element: symbol, index and y_hat (into its strided slot) of element i = (n, r) in one launch.
// `si`: x the step, y its inverse, here and below.
struct QCode {
  const float* y; const float* mu; const float* sc; const float* table;
  int* sym; int* idx; float* yh;
  int ns;
  float bound;
};
__device__ __forceinline__ void code_store(const QCode& o, const QGeom& g, long long n, long long r, long long i, int s,
                                           int ix, float m, float step) {
  o.sym[i] = s;
  o.idx[i] = ix;
  o.yh[n * g.yh_bs + r] = yh_of(s, m, step);
}
__device__ __forceinline__ void code_elem(const QCode& o, const QGeom& g, long long n, long long r, long long i,
                                          float2 si) {
  const float m = o.mu[n * g.mu_bs + r];
  const int s = symbol_of(o.y[n * g.y_bs + r], m, si.y);
  code_store(o, g, n, r, i, s, index_of(o.sc[n * g.sc_bs + r], o.bound, si.y, o.table, o.ns), m, si.x);
}

__global__ __launch_bounds__(256) void gc_code_q_kernel(const float* __restrict__ y, const float* __restrict__ mu,
                                                         const float* __restrict__ sc, const float* __restrict__ table,
                                                         int ns, float bound, float step, float inv,
                                                         int* __restrict__ sym, int* __restrict__ idx,
                                                         float* __restrict__ yh, const QGeom g) {
  const QCode o{y, mu, sc, table, sym, idx, yh, ns, bound};
  const long long per = (long long)g.C * g.HW, total = per * g.N;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / per, r = i - n * per;
    code_elem(o, g, n, r, i, make_float2(step, inv));
  }
}
__global__ __launch_bounds__(256) void gc_code_qmap_kernel(const float* __restrict__ y, const float* __restrict__ mu,
                                                            const float* __restrict__ sc,
                                                            const float* __restrict__ table, int ns, float bound,
                                                            const unsigned char* __restrict__ qmap,
                                                            const float2* __restrict__ steps, int* __restrict__ sym,
                                                            int* __restrict__ idx, float* __restrict__ yh,
                                                            const QGeom g) {
  const QCode o{y, mu, sc, table, sym, idx, yh, ns, bound};
  for (long long p = blockIdx.x * 256 + threadIdx.x; p < g.HW; p += gridDim.x * 256) {
    const float2 si = steps[qmap[p]];
    for (int n = blockIdx.z; n < g.N; n += gridDim.z) {
      for (int c = blockIdx.y; c < g.C; c += gridDim.y) {
        const long long r = (long long)c * g.HW + p;
        code_elem(o, g, n, r, (long long)n * g.C * g.HW + r, si);
      }
    }
  }
}

// ---- rate-distortion optimised quantisation: the encoder's element with a choice between the nearest symbol s0
// and its neighbour toward zero, s1 = s0 - sign(s0).  The coder tables say what each costs: `bits` has
// the shape of the CDF table, bits[r][v] = 16 - log2(cdf[r][v + 1] - cdf[r][v]) in f32, built on the host
// (icm_amd/bitstream.py: code_length_table), so nothing here is transcendental.  Per element, all f32, one rounding per
// operation:
//     u = (y - mu) * inv;  v_j = s_j - offsets[idx];  e_j = u - (float)s_j;  J_j = (w * (e_j * e_j)) + bits[idx][v_j]
// and s1 is coded iff s0 != 0, both v_j lie in the table proper, 0 .. cdf_sizes[idx] - 3 (an escaped symbol is never
// touched and none becomes one), and J1 < J0 strictly.  y_hat is that of the symbol coded (code_store); idx does not
// depend on it, so the decoder needs to know nothing.  With a weight so large that J1 < J0 never holds, the outputs are
// gc_code_q_kernel's / gc_code_qmap_kernel's bit for bit.
// One kernel for the scalar pair (`qmap` null) and the codec's map, on the z = n map grid in both forms: a map is read
// by position, the scalar form is the same loop with one pair for every position, and the 3-D grid is no slower (a
// kernel trace has this kernel at 10.4 us on the slice above, where the flat grid's cap of 256 workgroups holds the
// scalar kernel at 18.4 us), so a second copy of the decision on a flat grid would buy nothing.  Beside
// the map kernel's traffic a lane reads offsets[idx] and cdf_sizes[idx] (64 rows: cache-resident) and, where both
// candidates are in the table, two neighbouring entries of one bits row (a gather, mostly out of L2).  The row bound
// is also held to cdf_stride - 2, so no table the caller passes makes a lane read outside `bits`.
struct RdoTables {
  const int* sizes; const int* offsets; const float* bits;
  int stride;
  float w;
};

__global__ __launch_bounds__(256) void gc_code_rdo_kernel(const float* __restrict__ y, const float* __restrict__ mu,
                                                           const float* __restrict__ sc,
                                                           const float* __restrict__ table, int ns, float bound,
                                                           float step, float inv,
                                                           const unsigned char* __restrict__ qmap,
                                                           const float2* __restrict__ steps, const RdoTables t,
                                                           int* __restrict__ sym, int* __restrict__ idx,
                                                           float* __restrict__ yh, const QGeom g) {
  const QCode o{y, mu, sc, table, sym, idx, yh, ns, bound};
  const int n = blockIdx.z;
  for (long long p = blockIdx.x * 256 + threadIdx.x; p < g.HW; p += gridDim.x * 256) {
    const float2 si = qmap ? steps[qmap[p]] : make_float2(step, inv);
    for (int c = blockIdx.y; c < g.C; c += gridDim.y) {
      const long long r = (long long)c * g.HW + p;
      const float m = mu[n * g.mu_bs + r], yv = y[n * g.y_bs + r];
      const float u = mul_rn(yv - m, si.y);
      const int ix = index_of(sc[n * g.sc_bs + r], bound, si.y, table, ns);
      int s = symbol_of(yv, m, si.y);
      if (s != 0) {
        const int s1 = s > 0 ? s - 1 : s + 1;
        const int off = t.offsets[ix], ov = min(t.sizes[ix], t.stride) - 2;
        const int v0 = s - off, v1 = s1 - off;   // |s| <= 2^30 and a table offset is small: no overflow
        if (v0 >= 0 && v0 < ov && v1 >= 0 && v1 < ov) {
          const float* row = t.bits + (long long)ix * t.stride;
          const float e0 = add_rn(u, -(float)s), e1 = add_rn(u, -(float)s1);
          const float j0 = add_rn(mul_rn(t.w, mul_rn(e0, e0)), row[v0]);
          const float j1 = add_rn(mul_rn(t.w, mul_rn(e1, e1)), row[v1]);
          if (j1 < j0) s = s1;
        }
      }
      code_store(o, g, n, r, (long long)n * g.C * g.HW + r, s, ix, m, si.x);
    }
  }
}

// ---- the decoder's two kernels around the entropy decoder's run: scale -> indexes before it, symbols and mu -> y_hat
// after it, with the scalar pair (flat) and with the codec's map
__global__ __launch_bounds__(256) void gc_indexes_q_kernel(const float* __restrict__ sc, const float* __restrict__ table,
                                                            int ns, float bound, float inv, int* __restrict__ idx,
                                                            const QGeom g) {
  const long long per = (long long)g.C * g.HW, total = per * g.N;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / per, r = i - n * per;
    idx[i] = index_of(sc[n * g.sc_bs + r], bound, inv, table, ns);
  }
}
__global__ __launch_bounds__(256) void dequantize_q_kernel(const int* __restrict__ sym, const float* __restrict__ mu,
                                                            float step, float* __restrict__ yh, const QGeom g) {
  const long long per = (long long)g.C * g.HW, total = per * g.N;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / per, r = i - n * per;
    yh[n * g.yh_bs + r] = yh_of(sym[i], mu[n * g.mu_bs + r], step);
  }
}
__global__ __launch_bounds__(256) void gc_indexes_qmap_kernel(const float* __restrict__ sc,
                                                               const float* __restrict__ table, int ns, float bound,
                                                               const unsigned char* __restrict__ qmap,
                                                               const float2* __restrict__ steps,
                                                               int* __restrict__ idx, const QGeom g) {
  for (long long p = blockIdx.x * 256 + threadIdx.x; p < g.HW; p += gridDim.x * 256) {
    const float inv = steps[qmap[p]].y;
    for (int n = blockIdx.z; n < g.N; n += gridDim.z) {
      for (int c = blockIdx.y; c < g.C; c += gridDim.y) {
        const long long r = (long long)c * g.HW + p;
        idx[(long long)n * g.C * g.HW + r] = index_of(sc[n * g.sc_bs + r], bound, inv, table, ns);
      }
    }
  }
}
__global__ __launch_bounds__(256) void dequantize_qmap_kernel(const int* __restrict__ sym, const float* __restrict__ mu,
                                                               const unsigned char* __restrict__ qmap,
                                                               const float2* __restrict__ steps,
                                                               float* __restrict__ yh, const QGeom g) {
  for (long long p = blockIdx.x * 256 + threadIdx.x; p < g.HW; p += gridDim.x * 256) {
    const float step = steps[qmap[p]].x;
    for (int n = blockIdx.z; n < g.N; n += gridDim.z) {
      for (int c = blockIdx.y; c < g.C; c += gridDim.y) {
        const long long r = (long long)c * g.HW + p;
        yh[n * g.yh_bs + r] = yh_of(sym[(long long)n * g.C * g.HW + r], mu[n * g.mu_bs + r], step);
      }
    }
  }
}

// ---- training and estimation at a step: the likelihood of icm_gc_likelihood_ste_fwd / _bwd (entropy.hip) in symbol
// units.  Per element, all f32:
//     t = (y - mu) * inv;  s = symbol_of(y, mu, inv);  w = noise ? t + noise : (float)s      the noise is in symbol units
//     se = max(scale, scale_bound) * inv                                                     index_of's own expression
//     lik = max(Phi((1/2 - |w|) / se) - Phi((-1/2 - |w|) / se), lik_bound)
//     y_hat = yh_of(s, mu, step)                       the codec's y_hat bit for bit, whether or not there is noise
// and the backward is gc_bwd_tail (icm_common.h) at that w and se.  The _qs pair reads the pair of image n and walks
// the flat grid (qs_blocks); the _qm pair reads that of (n, p) from the trainer's map [N][HW] on the z = n map grid.
// Both call the element functions below, so a map that is uniform over an image gives that image the bits of the
// per-image pair.  `steps`: [N] pairs for _qs, the 256-pair table for _qm.
struct GcQsDesc {
  const float* y; const float* mu; const float* sc; const float* noise; const float2* steps;
  float* lik; float* yh; float* yh2;
  long long y_bs, mu_bs, sc_bs, nz_bs, lik_bs, yh_bs, yh2_bs;
  int N, C, HW;
  float scale_bound, lik_bound;
};
struct GcQsBwdDesc {
  const float* y; const float* mu; const float* sc; const float* noise; const float2* steps; const float* dlik;
  const float* dyh;
  float* dy; float* dmu; float* dsc;
  long long y_bs, mu_bs, sc_bs, nz_bs, dl_bs, dyh_bs, dy_bs, dmu_bs, dsc_bs;
  int N, C, HW, accum_dy;
  float scale_bound, lik_bound;
};

__device__ __forceinline__ void lik_fwd_elem(const GcQsDesc& d, long long n, long long r, float2 si) {
  const float y = d.y[n * d.y_bs + r], mu = d.mu[n * d.mu_bs + r], sc = d.sc[n * d.sc_bs + r];
  const int s = symbol_of(y, mu, si.y);
  const float w = d.noise ? mul_rn(y - mu, si.y) + d.noise[n * d.nz_bs + r] : (float)s;
  const float v = fabsf(w);
  const float se = mul_rn(fmaxf(sc, d.scale_bound), si.y);
  const float up = std_cdf((0.5f - v) / se), lo = std_cdf((-0.5f - v) / se);
  d.lik[n * d.lik_bs + r] = fmaxf(up - lo, d.lik_bound);
  const float yh = yh_of(s, mu, si.x);
  if (d.yh) d.yh[n * d.yh_bs + r] = yh;
  if (d.yh2) d.yh2[n * d.yh2_bs + r] = yh;
}
__device__ __forceinline__ void lik_bwd_elem(const GcQsBwdDesc& d, long long n, long long r, float inv) {
  const float y = d.y[n * d.y_bs + r], mu = d.mu[n * d.mu_bs + r], sc = d.sc[n * d.sc_bs + r];
  const float w = d.noise ? mul_rn(y - mu, inv) + d.noise[n * d.nz_bs + r] : (float)symbol_of(y, mu, inv);
  gc_bwd_tail(d, n, r, w, mul_rn(fmaxf(sc, d.scale_bound), inv), sc, inv);
}

__global__ __launch_bounds__(256) void gc_qs_fwd_kernel(const GcQsDesc d) {
  const long long per = (long long)d.C * d.HW, total = per * d.N;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / per, r = i - n * per;
    lik_fwd_elem(d, n, r, d.steps[n]);
  }
}
__global__ __launch_bounds__(256) void gc_qs_bwd_kernel(const GcQsBwdDesc d) {
  const long long per = (long long)d.C * d.HW, total = per * d.N;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / per, r = i - n * per;
    lik_bwd_elem(d, n, r, d.steps[n].y);
  }
}
__global__ __launch_bounds__(256) void gc_qm_fwd_kernel(const GcQsDesc d, const unsigned char* __restrict__ qmap) {
  const int n = blockIdx.z;
  for (long long p = blockIdx.x * 256 + threadIdx.x; p < d.HW; p += gridDim.x * 256) {
    const float2 si = d.steps[qmap[(long long)n * d.HW + p]];
    for (int c = blockIdx.y; c < d.C; c += gridDim.y) lik_fwd_elem(d, n, (long long)c * d.HW + p, si);
  }
}
__global__ __launch_bounds__(256) void gc_qm_bwd_kernel(const GcQsBwdDesc d, const unsigned char* __restrict__ qmap) {
  const int n = blockIdx.z;
  for (long long p = blockIdx.x * 256 + threadIdx.x; p < d.HW; p += gridDim.x * 256) {
    const float inv = d.steps[qmap[(long long)n * d.HW + p]].y;
    for (int c = blockIdx.y; c < d.C; c += gridDim.y) lik_bwd_elem(d, n, (long long)c * d.HW + p, inv);
  }
}

// ---- painting the training maps on the device: qmap [N][h][w] int8; every cell of image n holds base[n], then the R
// rectangles rects[n][r] = (y0, x0, y1, x1, k) (cells, half open) are painted in order, later ones winning
// (icm_amd/codec.py: roi_map).  One lane per cell walks the image's rectangles (paint_cell: R is small and the reads
// are wave-uniform) and stores once; a rectangle is clipped to the map by the test itself, an empty one holds no cell.
// grid (blocks over h * w, N); k and the coordinates are not range-checked.
__device__ __forceinline__ int paint_cell(int k, const int* __restrict__ rn, int R, int cy, int cx) {
  for (int r = 0; r < R; ++r) {
    const int* q = rn + 5 * r;
    if (cy >= q[0] && cx >= q[1] && cy < q[2] && cx < q[3]) k = q[4];
  }
  return k;
}
__global__ __launch_bounds__(256) void qmap_paint_kernel(const signed char* __restrict__ base,
                                                          const int* __restrict__ rects, int R, int h, int w,
                                                          signed char* __restrict__ qmap) {
  const int n = blockIdx.y, hw = h * w;
  const int* rn = rects + (long long)n * R * 5;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < hw; p += gridDim.x * 256) {   // hw <= 2^30: no overflow
    const int cy = p / w, cx = p - cy * w;
    qmap[(long long)n * hw + p] = (signed char)paint_cell(base[n], rn, R, cy, cx);
  }
}

// ---- the maps of variance-adaptive quantisation for a training batch (icm_qmap_aq): what icm_amd/codec.py makes of
// an image for `codec encode --aq S` (cell_stats, aq_activity, aq_reference, aq_offsets, quality_map), restated for
// planar f32 crops [N][3][H][W] of whole 16 x 16 cells, so n = 256 in every cell and nothing is padding.  Two launches:
//
//   qmap_aq_activity_kernel   a wave per cell: lane l owns four pixels of row l / 4 (three 16-byte loads, one per
//       plane; the four lanes of a row read its 64 contiguous bytes, the four waves of a workgroup four neighbouring
//       cells).  A sample's 8-bit value is quantise_u8 (image_u8.h: the codec's own rule), Y = (77 R + 150 G + 29 B +
//       128) >> 8, and s1 = sum Y, s2 = sum Y^2 are integers added across the wave by shuffles: exact in any order.
//       Lane 0 forms 256 s2 - s1^2 in 64 bits (it passes 2^32), v = that / 65536 (exact in double) and stores
//       L = log2(1 + v) in DOUBLE into act [N][h w]: a batch has a few thousand cells, and the double is what lets a
//       test ask for the map cell by cell.
//   qmap_aq_map_kernel        a workgroup per image.  ref[n] = mean of L over the image's cells, summed in double in an
//       order fixed by the cell index alone: partial j = L[j] + L[j + 256] + ... in ascending order, then the binary
//       tree red[t] += red[t + m], m = 128 .. 1, over the 256 partials; no atomics, the same bits on every run and in
//       every batch.  Then per cell d = clip(rint(4 (double)strength[n] (L - ref[n])), -16, 16) (v_rndne: ties to
//       even), k = clamp(base[n] + d, -16, 32), and the image's rectangles over it (paint_cell); one store per cell.
//
// Every entry of qmap and ref is written once and act is written before it is read, so nothing needs clearing.
constexpr int AQ_CELL = 16;
constexpr int AQ_K_MIN = -16, AQ_K_MAX = 32;   // bitstream.py: QSTEP_MIN, QSTEP_MAX
constexpr double AQ_MAX_OFFSET = 16.0;         // codec.py: AQ_MAX_OFFSET

__global__ __launch_bounds__(256) void qmap_aq_activity_kernel(const float* __restrict__ x, int H, int W, int w,
                                                                long long per, long long cells,
                                                                double* __restrict__ act) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, row = lane >> 2, q4 = (lane & 3) * 4;
  const long long plane = (long long)H * W;
  for (long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); c < cells; c += (long long)gridDim.x * 4) {
    const long long n = c / per;
    const int p = (int)(c - n * per), cy = p / w, cx = p - cy * w;
    const float* px = x + n * 3 * plane + (long long)(cy * AQ_CELL + row) * W + cx * AQ_CELL + q4;
    const f32x4 r = *reinterpret_cast<const f32x4*>(px);
    const f32x4 g = *reinterpret_cast<const f32x4*>(px + plane);
    const f32x4 b = *reinterpret_cast<const f32x4*>(px + 2 * plane);
    int s1 = 0, s2 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int Y = (int)((77u * quantise_u8(r[j]) + 150u * quantise_u8(g[j]) + 29u * quantise_u8(b[j]) + 128u) >> 8);
      s1 += Y;
      s2 += Y * Y;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {   // c is wave-uniform: all 64 lanes are here
      s1 += __shfl_xor(s1, m, 64);
      s2 += __shfl_xor(s2, m, 64);
    }
    if (lane == 0) {
      const long long num = 256LL * s2 - (long long)s1 * s1;
      act[c] = log2(1.0 + (double)num / 65536.0);
    }
  }
}

__global__ __launch_bounds__(256) void qmap_aq_map_kernel(const double* __restrict__ act,
                                                           const signed char* __restrict__ base,
                                                           const float* __restrict__ strength,
                                                           const int* __restrict__ rects, int R, int h, int w,
                                                           signed char* __restrict__ qmap, double* __restrict__ ref) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const int n = blockIdx.x, hw = h * w, t = threadIdx.x;   // hw <= 2^30: p + 256 stays an int
  const double* a = act + (long long)n * hw;
  const int* rn = rects + (long long)n * R * 5;
  double s = 0.0;
  for (int p = t; p < hw; p += 256) s += a[p];
  red[t] = s;
  __syncthreads();
  for (int m = 128; m > 0; m >>= 1) {
    if (t < m) red[t] += red[t + m];
    __syncthreads();
  }
  const double mean = red[0] / (double)hw;
  if (t == 0) ref[n] = mean;
  const double gain = 4.0 * (double)strength[n];
  const int b = base[n];
  for (int p = t; p < hw; p += 256) {
    const int cy = p / w, cx = p - cy * w;
    const double d = fmin(fmax(rint(gain * (a[p] - mean)), -AQ_MAX_OFFSET), AQ_MAX_OFFSET);
    const int k = min(max(b + (int)d, AQ_K_MIN), AQ_K_MAX);
    qmap[(long long)n * hw + p] = (signed char)paint_cell(k, rn, R, cy, cx);
  }
}

}  // namespace icm

using namespace icm;

// every pointer an entry point requires is set and the three extents are positive; what else an entry point rejects
// stands in that entry point
static inline bool args_ok(std::initializer_list<const void*> ptrs, int N, int C, int HW) {
  for (const void* p : ptrs)
    if (!p) return false;
  return N >= 1 && C >= 1 && HW >= 1;
}
static inline bool step_ok(float v) { return std::isfinite(v) && v > 0.0f; }
static inline int q_blocks(long long total) {
  return (int)std::max<long long>(1, std::min<long long>((total + 255) / 256, 256));
}
// the flat grid of the training pair: a training slice of a 16 x 256 x 256 batch has 131 072 elements
static inline int qs_blocks(long long total) {
  return (int)std::max<long long>(1, std::min<long long>((total + 255) / 256, 2048));
}
// grid of the map kernels: x covers HW in 256-lane blocks, then c and n share what is left of QMAP_BLOCKS workgroups
// (four per CU: each walks a few channels with its positions' pairs in registers)
constexpr int QMAP_BLOCKS = 1024;
static inline dim3 qmap_grid(int N, int C, int HW) {
  const int gx = std::min((HW - 1) / 256 + 1, QMAP_BLOCKS);
  const int gy = std::min(C, std::max(1, QMAP_BLOCKS / gx));
  const int gz = std::min(N, std::max(1, QMAP_BLOCKS / (gx * gy)));
  return dim3(gx, gy, gz);
}
// the z = n form: qmap_grid's x and y (a grid's z holds 65 535)
constexpr int QM_MAX_N = 65535;
static inline dim3 qm_grid(int N, int C, int HW) {
  const dim3 g = qmap_grid(1, C, HW);
  return dim3(g.x, g.y, N);
}

// the training pair behind its _qs (`qmap` null: `pairs` [N]) and _qm (`pairs` the table) entry points
static int lik_fwd(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale, int64_t sc_bs,
                   const float* noise, int64_t nz_bs, const float* pairs, const int8_t* qmap, float* lik, int64_t lik_bs,
                   float* yh, int64_t yh_bs, float* yh2, int64_t yh2_bs, int N, int C, int HW, float scale_bound,
                   float lik_bound, void* stream) {
  if (!args_ok({y, mu, scale, pairs, lik}, N, C, HW) || scale_bound <= 0) return ICM_ERR_ARG;
  const GcQsDesc d{y, mu, scale, noise, (const float2*)pairs, lik, yh, yh2, y_bs, mu_bs, sc_bs, nz_bs, lik_bs, yh_bs,
                   yh2_bs, N, C, HW, scale_bound, lik_bound};
  if (qmap)
    hipLaunchKernelGGL(gc_qm_fwd_kernel, qm_grid(N, C, HW), dim3(256), 0, (hipStream_t)stream, d,
                       (const unsigned char*)qmap);
  else
    hipLaunchKernelGGL(gc_qs_fwd_kernel, dim3(qs_blocks((long long)N * C * HW)), dim3(256), 0, (hipStream_t)stream, d);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}
static int lik_bwd(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale, int64_t sc_bs,
                   const float* noise, int64_t nz_bs, const float* pairs, const int8_t* qmap, const float* dlik,
                   int64_t dl_bs, const float* dyh, int64_t dyh_bs, float* dy, int64_t dy_bs, float* dmu, int64_t dmu_bs,
                   float* dscale, int64_t dsc_bs, int N, int C, int HW, float scale_bound, float lik_bound, int accum_dy,
                   void* stream) {
  if (!args_ok({y, mu, scale, pairs, dlik, dy, dmu, dscale}, N, C, HW)) return ICM_ERR_ARG;
  const GcQsBwdDesc d{y, mu, scale, noise, (const float2*)pairs, dlik, dyh, dy, dmu, dscale, y_bs, mu_bs, sc_bs, nz_bs,
                      dl_bs, dyh_bs, dy_bs, dmu_bs, dsc_bs, N, C, HW, accum_dy, scale_bound, lik_bound};
  if (qmap)
    hipLaunchKernelGGL(gc_qm_bwd_kernel, qm_grid(N, C, HW), dim3(256), 0, (hipStream_t)stream, d,
                       (const unsigned char*)qmap);
  else
    hipLaunchKernelGGL(gc_qs_bwd_kernel, dim3(qs_blocks((long long)N * C * HW)), dim3(256), 0, (hipStream_t)stream, d);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

extern "C" {

int icm_gc_code_q(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale, int64_t sc_bs,
                  const float* scale_table, int ns, float scale_bound, float step, float inv, int32_t* symbols,
                  int32_t* indexes, float* yh, int64_t yh_bs, int N, int C, int HW, void* stream) {
  if (!args_ok({y, mu, scale, scale_table, symbols, indexes, yh}, N, C, HW)) return ICM_ERR_ARG;
  if (!step_ok(step) || !step_ok(inv) || ns < 1) return ICM_ERR_ARG;
  const QGeom g{y_bs, mu_bs, sc_bs, yh_bs, N, C, HW};
  hipLaunchKernelGGL(gc_code_q_kernel, dim3(q_blocks((long long)N * C * HW)), dim3(256), 0, (hipStream_t)stream, y, mu,
                     scale, scale_table, ns, scale_bound, step, inv, symbols, indexes, yh, g);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_gc_indexes_q(const float* scale, int64_t sc_bs, const float* scale_table, int ns, float scale_bound, float inv,
                     int32_t* indexes, int N, int C, int HW, void* stream) {
  if (!args_ok({scale, scale_table, indexes}, N, C, HW) || !step_ok(inv) || ns < 1) return ICM_ERR_ARG;
  const QGeom g{0, 0, sc_bs, 0, N, C, HW};
  hipLaunchKernelGGL(gc_indexes_q_kernel, dim3(q_blocks((long long)N * C * HW)), dim3(256), 0, (hipStream_t)stream,
                     scale, scale_table, ns, scale_bound, inv, indexes, g);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_dequantize_q(const int32_t* symbols, const float* mu, int64_t mu_bs, float step, float* yh, int64_t yh_bs, int N,
                     int C, int HW, void* stream) {
  if (!args_ok({symbols, mu, yh}, N, C, HW) || !step_ok(step)) return ICM_ERR_ARG;
  const QGeom g{0, mu_bs, 0, yh_bs, N, C, HW};
  hipLaunchKernelGGL(dequantize_q_kernel, dim3(q_blocks((long long)N * C * HW)), dim3(256), 0, (hipStream_t)stream,
                     symbols, mu, step, yh, g);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_gc_code_qmap(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale, int64_t sc_bs,
                     const float* scale_table, int ns, float scale_bound, const int8_t* qmap, const float* step_table,
                     int32_t* symbols, int32_t* indexes, float* yh, int64_t yh_bs, int N, int C, int HW, void* stream) {
  if (!args_ok({y, mu, scale, scale_table, qmap, step_table, symbols, indexes, yh}, N, C, HW) || ns < 1)
    return ICM_ERR_ARG;
  const QGeom g{y_bs, mu_bs, sc_bs, yh_bs, N, C, HW};
  hipLaunchKernelGGL(gc_code_qmap_kernel, qmap_grid(N, C, HW), dim3(256), 0, (hipStream_t)stream, y, mu, scale,
                     scale_table, ns, scale_bound, (const unsigned char*)qmap, (const float2*)step_table, symbols,
                     indexes, yh, g);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_gc_code_rdo(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale, int64_t sc_bs,
                    const float* scale_table, int ns, float scale_bound, float step, float inv, const int8_t* qmap,
                    const float* step_table, const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes,
                    const int32_t* offsets, int ncdf, const float* bits, float w, int32_t* symbols, int32_t* indexes,
                    float* yh, int64_t yh_bs, int N, int C, int HW, void* stream) {
  if (!args_ok({y, mu, scale, scale_table, symbols, indexes, yh, cdfs, cdf_sizes, offsets, bits}, N, C, HW))
    return ICM_ERR_ARG;
  if ((qmap == nullptr) != (step_table == nullptr)) return ICM_ERR_ARG;
  if (!step_ok(step) || !step_ok(inv) || !step_ok(w)) return ICM_ERR_ARG;
  if (ns < 1 || ns != ncdf || cdf_stride < 3 || N > QM_MAX_N) return ICM_ERR_ARG;
  const QGeom g{y_bs, mu_bs, sc_bs, yh_bs, N, C, HW};
  const RdoTables t{cdf_sizes, offsets, bits, cdf_stride, w};
  hipLaunchKernelGGL(gc_code_rdo_kernel, qm_grid(N, C, HW), dim3(256), 0, (hipStream_t)stream, y, mu, scale,
                     scale_table, ns, scale_bound, step, inv, (const unsigned char*)qmap, (const float2*)step_table, t,
                     symbols, indexes, yh, g);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_gc_indexes_qmap(const float* scale, int64_t sc_bs, const float* scale_table, int ns, float scale_bound,
                        const int8_t* qmap, const float* step_table, int32_t* indexes, int N, int C, int HW,
                        void* stream) {
  if (!args_ok({scale, scale_table, qmap, step_table, indexes}, N, C, HW) || ns < 1) return ICM_ERR_ARG;
  const QGeom g{0, 0, sc_bs, 0, N, C, HW};
  hipLaunchKernelGGL(gc_indexes_qmap_kernel, qmap_grid(N, C, HW), dim3(256), 0, (hipStream_t)stream, scale, scale_table,
                     ns, scale_bound, (const unsigned char*)qmap, (const float2*)step_table, indexes, g);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_dequantize_qmap(const int32_t* symbols, const float* mu, int64_t mu_bs, const int8_t* qmap,
                        const float* step_table, float* yh, int64_t yh_bs, int N, int C, int HW, void* stream) {
  if (!args_ok({symbols, mu, qmap, step_table, yh}, N, C, HW)) return ICM_ERR_ARG;
  const QGeom g{0, mu_bs, 0, yh_bs, N, C, HW};
  hipLaunchKernelGGL(dequantize_qmap_kernel, qmap_grid(N, C, HW), dim3(256), 0, (hipStream_t)stream, symbols, mu,
                     (const unsigned char*)qmap, (const float2*)step_table, yh, g);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_gc_likelihood_ste_qs_fwd(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale,
                                 int64_t sc_bs, const float* noise, int64_t nz_bs, const float* steps, float* lik,
                                 int64_t lik_bs, float* yh, int64_t yh_bs, float* yh2, int64_t yh2_bs, int N, int C,
                                 int HW, float scale_bound, float lik_bound, void* stream) {
  return lik_fwd(y, y_bs, mu, mu_bs, scale, sc_bs, noise, nz_bs, steps, nullptr, lik, lik_bs, yh, yh_bs, yh2, yh2_bs, N,
                 C, HW, scale_bound, lik_bound, stream);
}

int icm_gc_likelihood_ste_qs_bwd(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale,
                                 int64_t sc_bs, const float* noise, int64_t nz_bs, const float* steps, const float* dlik,
                                 int64_t dl_bs, const float* dyh, int64_t dyh_bs, float* dy, int64_t dy_bs, float* dmu,
                                 int64_t dmu_bs, float* dscale, int64_t dsc_bs, int N, int C, int HW, float scale_bound,
                                 float lik_bound, int accum_dy, void* stream) {
  return lik_bwd(y, y_bs, mu, mu_bs, scale, sc_bs, noise, nz_bs, steps, nullptr, dlik, dl_bs, dyh, dyh_bs, dy, dy_bs,
                 dmu, dmu_bs, dscale, dsc_bs, N, C, HW, scale_bound, lik_bound, accum_dy, stream);
}

int icm_gc_likelihood_ste_qm_fwd(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale,
                                 int64_t sc_bs, const float* noise, int64_t nz_bs, const int8_t* qmap,
                                 const float* step_table, float* lik, int64_t lik_bs, float* yh, int64_t yh_bs,
                                 float* yh2, int64_t yh2_bs, int N, int C, int HW, float scale_bound, float lik_bound,
                                 void* stream) {
  if (!qmap || N > QM_MAX_N) return ICM_ERR_ARG;
  return lik_fwd(y, y_bs, mu, mu_bs, scale, sc_bs, noise, nz_bs, step_table, qmap, lik, lik_bs, yh, yh_bs, yh2, yh2_bs,
                 N, C, HW, scale_bound, lik_bound, stream);
}

int icm_gc_likelihood_ste_qm_bwd(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale,
                                 int64_t sc_bs, const float* noise, int64_t nz_bs, const int8_t* qmap,
                                 const float* step_table, const float* dlik, int64_t dl_bs, const float* dyh,
                                 int64_t dyh_bs, float* dy, int64_t dy_bs, float* dmu, int64_t dmu_bs, float* dscale,
                                 int64_t dsc_bs, int N, int C, int HW, float scale_bound, float lik_bound, int accum_dy,
                                 void* stream) {
  if (!qmap || N > QM_MAX_N) return ICM_ERR_ARG;
  return lik_bwd(y, y_bs, mu, mu_bs, scale, sc_bs, noise, nz_bs, step_table, qmap, dlik, dl_bs, dyh, dyh_bs, dy, dy_bs,
                 dmu, dmu_bs, dscale, dsc_bs, N, C, HW, scale_bound, lik_bound, accum_dy, stream);
}

int icm_qmap_paint(const int8_t* base, const int32_t* rects, int R, int8_t* qmap, int N, int h, int w, void* stream) {
  if (!args_ok({base, rects, qmap}, N, h, w) || R < 0) return ICM_ERR_ARG;
  if ((long long)h * w > (1LL << 30) || N > 65535) return ICM_ERR_ARG;   // int cell indexes; N is the grid's y
  const int gx = (int)std::min<long long>(((long long)h * w + 255) / 256, 1024);
  hipLaunchKernelGGL(qmap_paint_kernel, dim3(gx, N), dim3(256), 0, (hipStream_t)stream, (const signed char*)base, rects,
                     R, h, w, (signed char*)qmap);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int64_t icm_qmap_aq_workspace_bytes(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1 || H % AQ_CELL || W % AQ_CELL) return 0;
  const long long hw = (long long)(H / AQ_CELL) * (W / AQ_CELL);
  if (hw > (1LL << 30) || N > 65535) return 0;
  return (int64_t)N * hw * (int64_t)sizeof(double);
}

int icm_qmap_aq(const float* x, int N, int H, int W, const int8_t* base, const float* strength, const int32_t* rects,
                int R, int8_t* qmap, double* ref, void* ws, int64_t ws_bytes, void* stream) {
  if (!args_ok({x, base, strength, qmap, ref, ws}, N, H, W) || R < 0 || (R > 0 && !rects)) return ICM_ERR_ARG;
  const int64_t need = icm_qmap_aq_workspace_bytes(N, H, W);   // 0: no whole cells, or icm_qmap_paint's limits
  if (need == 0 || ws_bytes < need) return ICM_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(x) & 15) || ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(ref)) & 7))
    return ICM_ERR_ARG;   // 16-byte loads of whole cell rows (W is a multiple of 16 floats); doubles
  const int h = H / AQ_CELL, w = W / AQ_CELL;
  const long long per = (long long)h * w, cells = per * N;
  const int gx = (int)std::min<long long>((cells + 3) / 4, 65536);
  hipLaunchKernelGGL(qmap_aq_activity_kernel, dim3(gx), dim3(256), 0, (hipStream_t)stream, x, H, W, w, per, cells,
                     (double*)ws);
  ICM_CHECK_LAUNCH();
  hipLaunchKernelGGL(qmap_aq_map_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, (const double*)ws,
                     (const signed char*)base, strength, rects, R, h, w, (signed char*)qmap, ref);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

}  // extern "C"
