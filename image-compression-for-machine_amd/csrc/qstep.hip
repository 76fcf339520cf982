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
// The decoder has the integer symbol, mu and scale, and must arrive at the encoder's y_hat and index bit for bit:
// `yh_of` and `index_of` are the only statements of those two expressions, and the encoder's fused kernel and the
// decoder's two kernels all call them.  (y_hat is formed from the symbol after its trip through int, in the encoder
// too, so a -0 of rint is the +0 the decoder sees.)  With step = inv = 1 the symbols are icm_quantize's, the indexes
// icm_gc_build_indexes' and y_hat the fused forward's.
//
// Memory-bound elementwise work on [N][C][HW] operands that are channel slices of wider buffers (an element batch
// stride per float operand; the int32 outputs are dense): one element per lane and pass, consecutive lanes on
// consecutive addresses, a grid-stride loop.  The table index j is wave-uniform, so the 64-entry table is read
// through the scalar cache; no LDS.  A slice of the largest image one compress() call takes has under a million
// elements: the grid is capped at one 256-thread workgroup per CU, which covers it in a few passes (measured: 19 us
// for the fused kernel on the 786 432 elements of a 2048x3072 image's slice, against 45 us for the three launches it
// replaces).
//
// Rate-distortion optimised quantisation (icm_gc_code_rdo) is the same fused launch with a choice of symbol, for the
// scalar pair and for a quality map alike.  It runs on the map kernels' 3-D grid (x over HW, y over c, z over n) in
// both forms, not on the flat grid above: a map is read by position, which the 3-D grid never divides out of a flat
// index, the scalar form is the same loop with one pair for every position, and the 3-D grid is no slower (a kernel
// trace has this kernel at 10.4 us on the slice above, where the flat grid's cap of 256 workgroups holds the scalar
// kernel at 18.4 us), so a second copy of the decision on a flat grid would buy nothing.
#include <algorithm>
#include <cmath>
#include "icm_common.h"

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

// encoder: symbols, indexes and y_hat (into its strided slot) of one slice in one launch
__global__ __launch_bounds__(256) void gc_code_q_kernel(const float* __restrict__ y, const float* __restrict__ mu,
                                                         const float* __restrict__ sc, const float* __restrict__ table,
                                                         int ns, float bound, float step, float inv,
                                                         int* __restrict__ sym, int* __restrict__ idx,
                                                         float* __restrict__ yh, const QGeom g) {
  const long long per = (long long)g.C * g.HW, total = per * g.N;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / per, r = i - n * per;
    const float m = mu[n * g.mu_bs + r];
    const int s = symbol_of(y[n * g.y_bs + r], m, inv);
    sym[i] = s;
    idx[i] = index_of(sc[n * g.sc_bs + r], bound, inv, table, ns);
    yh[n * g.yh_bs + r] = yh_of(s, m, step);
  }
}
// decoder, before the entropy decoder's run: scale -> indexes
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
// decoder, after it: symbols, mu -> y_hat
__global__ __launch_bounds__(256) void dequantize_q_kernel(const int* __restrict__ sym, const float* __restrict__ mu,
                                                            float step, float* __restrict__ yh, const QGeom g) {
  const long long per = (long long)g.C * g.HW, total = per * g.N;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / per, r = i - n * per;
    yh[n * g.yh_bs + r] = yh_of(sym[i], mu[n * g.mu_bs + r], step);
  }
}

// ---- quality map: a step per latent position.  `qmap` holds HW step indexes k (int8, dense, shared by every n and c),
// `steps` 256 (step, inv) pairs indexed by the map byte read as unsigned (icm_amd/bitstream.py: step_table; bytes that
// are no valid k hold (1, 1), so no byte indexes outside it and nothing here clamps or branches on validity).  The
// arithmetic is symbol_of / yh_of / index_of above, called with the pair of the element's position.
// Layout: a 3-D grid, x over HW, y over c, z over n, each a grid-stride loop, so a position index is never divided
// out of a flat one.  A lane reads its map byte and its pair once per position (consecutive lanes on consecutive map
// bytes: 64 bytes per wave) and keeps them in registers over the channels and images it walks; the operand accesses
// stay consecutive lanes on consecutive addresses.  `se` differs per lane now, table[j] is still wave-uniform and
// still comes through the scalar cache.  The pairs are read with plain global loads (one 8-byte load per lane and
// position; the table is 2 KB, read-only and stays in cache); the plain form is the one kept and an LDS-staged
// table was not needed: on the 786 432-element slice the fused map kernel measured 19.9 - 20.0 us against the scalar
// kernel's 19.5 - 19.9 us in the same run.
__global__ __launch_bounds__(256) void gc_code_qmap_kernel(const float* __restrict__ y, const float* __restrict__ mu,
                                                            const float* __restrict__ sc,
                                                            const float* __restrict__ table, int ns, float bound,
                                                            const unsigned char* __restrict__ qmap,
                                                            const float2* __restrict__ steps, int* __restrict__ sym,
                                                            int* __restrict__ idx, float* __restrict__ yh,
                                                            const QGeom g) {
  for (long long p = blockIdx.x * 256 + threadIdx.x; p < g.HW; p += gridDim.x * 256) {
    const float2 si = steps[qmap[p]];   // x: step, y: inv
    for (int n = blockIdx.z; n < g.N; n += gridDim.z) {
      for (int c = blockIdx.y; c < g.C; c += gridDim.y) {
        const long long r = (long long)c * g.HW + p;
        const long long i = (long long)n * g.C * g.HW + r;
        const float m = mu[n * g.mu_bs + r];
        const int s = symbol_of(y[n * g.y_bs + r], m, si.y);
        sym[i] = s;
        idx[i] = index_of(sc[n * g.sc_bs + r], bound, si.y, table, ns);
        yh[n * g.yh_bs + r] = yh_of(s, m, si.x);
      }
    }
  }
}
// ---- rate-distortion optimised quantisation: the encoder's fused launch with a choice between the nearest symbol s0
// and its neighbour toward zero, s1 = s0 - sign(s0).  The coder tables say what each costs: `bits` has
// the shape of the CDF table, bits[r][v] = 16 - log2(cdf[r][v + 1] - cdf[r][v]) in f32, built on the host
// (icm_amd/bitstream.py: code_length_table), so nothing here is transcendental.  Per element, all f32, one rounding per
// operation:
//     u = (y - mu) * inv;  v_j = s_j - offsets[idx];  e_j = u - (float)s_j;  J_j = (w * (e_j * e_j)) + bits[idx][v_j]
// and s1 is coded iff s0 != 0, both v_j lie in the table proper, 0 .. cdf_sizes[idx] - 3 (an escaped symbol is never
// touched and none becomes one), and J1 < J0 strictly.  y_hat is yh_of of the symbol coded; idx does not depend on it,
// so the decoder needs to know nothing.  symbol_of / index_of / yh_of are the ones above: with a weight so large that
// J1 < J0 never holds, the outputs are gc_code_q_kernel's / gc_code_qmap_kernel's bit for bit.
// Layout: the map kernels' 3-D grid for both forms (`qmap` null: the scalar pair for every position), with z the
// image itself as in gc_qm_fwd_kernel (qm_grid: a codec batch is small, and with n fixed per workgroup the operand
// offsets n * bs fold into the base pointers; with a loop over n the kernel spilled scalar registers).  The scalar
// kernel's flat grid would have to divide the position out of the flat index to read a map; here the pair is read
// once per position and held over the channels, and one kernel serves both.  Consecutive lanes on consecutive addresses in every operand.  Beside the
// map kernel's traffic a lane reads offsets[idx] and cdf_sizes[idx] (64 rows: cache-resident) and, where both
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
  const int n = blockIdx.z;
  for (long long p = blockIdx.x * 256 + threadIdx.x; p < g.HW; p += gridDim.x * 256) {
    const float2 si = qmap ? steps[qmap[p]] : make_float2(step, inv);   // x: step, y: inv
    for (int c = blockIdx.y; c < g.C; c += gridDim.y) {
      const long long r = (long long)c * g.HW + p;
      const long long i = (long long)n * g.C * g.HW + r;
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
      sym[i] = s;
      idx[i] = ix;
      yh[n * g.yh_bs + r] = yh_of(s, m, si.x);
    }
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
// units, with a (step, inv) pair per IMAGE read from device memory (`steps` [N] float2: a captured training graph is
// replayed with fresh steps).  Per element of image n, all f32:
//     t = (y - mu) * inv;  s = symbol_of(y, mu, inv);  v = noise ? t + noise : (float)s      the noise is in symbol units
//     se = max(scale, scale_bound) * inv                                                     index_of's own expression
//     lik = max(Phi((1/2 - |v|) / se) - Phi((-1/2 - |v|) / se), lik_bound)
//     y_hat = yh_of(s, mu, step)                       the codec's y_hat bit for bit, whether or not there is noise
// Backward, with pu / pl the densities at the two arguments u, l:  d lik / d|v| = (pl - pu) / se,
// d lik / d se = (l pl - u pu) / se;  dv / dy = -dv / dmu = inv (with noise; the rounded symbol passes nothing),
// d se / d scale = inv above the scale bound.  The two LowerBound gates are gc_bwd_kernel's: a gradient passes a bound
// that is active only if it pushes the value up.  d y_hat passes to y unchanged (straight-through) and not to mu.
// The same grid-stride shape as the scalar pair: the pair of image n is a wave-uniform 8-byte load per element (N
// pairs: they stay in cache).
struct GcQsDesc {
  const float* y; const float* mu; const float* sc; const float* noise; const float2* steps;
  float* lik; float* yh; float* yh2;
  long long y_bs, mu_bs, sc_bs, nz_bs, lik_bs, yh_bs, yh2_bs;
  int N, C, HW;
  float scale_bound, lik_bound;
};

__global__ __launch_bounds__(256) void gc_qs_fwd_kernel(const GcQsDesc d) {
  const long long per = (long long)d.C * d.HW, total = per * d.N;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / per, r = i - n * per;
    const float2 si = d.steps[n];   // x: step, y: inv
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
}

struct GcQsBwdDesc {
  const float* y; const float* mu; const float* sc; const float* noise; const float2* steps; const float* dlik;
  const float* dyh;
  float* dy; float* dmu; float* dsc;
  long long y_bs, mu_bs, sc_bs, nz_bs, dl_bs, dyh_bs, dy_bs, dmu_bs, dsc_bs;
  int N, C, HW, accum_dy;
  float scale_bound, lik_bound;
};

__global__ __launch_bounds__(256) void gc_qs_bwd_kernel(const GcQsBwdDesc d) {
  const long long per = (long long)d.C * d.HW, total = per * d.N;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / per, r = i - n * per;
    const float inv = d.steps[n].y;
    const float y = d.y[n * d.y_bs + r], mu = d.mu[n * d.mu_bs + r], sc = d.sc[n * d.sc_bs + r];
    const float w = d.noise ? mul_rn(y - mu, inv) + d.noise[n * d.nz_bs + r] : (float)symbol_of(y, mu, inv);
    const float v = fabsf(w);
    const float se = mul_rn(fmaxf(sc, d.scale_bound), inv);
    const float u = (0.5f - v) / se, l = (-0.5f - v) / se;
    const float lraw = std_cdf(u) - std_cdf(l);
    float g = d.dlik[n * d.dl_bs + r];
    if (!(lraw >= d.lik_bound || g < 0.0f)) g = 0.0f;
    const float pu = std_pdf(u), pl = std_pdf(l);
    const float dv = g * (pl - pu) / se;
    float gs = g * (l * pl - u * pu) / se * inv;
    if (!(sc >= d.scale_bound || gs < 0.0f)) gs = 0.0f;
    const float sg = w > 0.0f ? 1.0f : (w < 0.0f ? -1.0f : 0.0f);
    float gy = 0.0f, gmu = 0.0f;
    if (d.noise) {
      gy = dv * sg * inv;
      gmu = -gy;
    }
    if (d.dyh) gy += d.dyh[n * d.dyh_bs + r];
    float* dyp = d.dy + n * d.dy_bs + r;
    if (d.accum_dy) gy += *dyp;
    *dyp = gy;
    d.dmu[n * d.dmu_bs + r] = gmu;
    d.dsc[n * d.dsc_bs + r] = gs;
  }
}

// ---- the same pair with a step per (image, position): quality-map training.  `qmap` [N][HW] int8 holds a step index
// per image and latent position, shared by the channels; `d.steps` is the 256-pair table of the codec's map kernels,
// indexed by the map byte read as unsigned (nothing here clamps the byte or branches on its validity).  Per element
// the arithmetic is gc_qs_fwd_kernel's / gc_qs_bwd_kernel's, statement for statement, with the pair of the element's
// position, so a map that is uniform over an image gives that image the bits of the per-image pair.
// Layout: that of the codec's map kernels (qmap_grid: x over HW, y over c, both grid-stride loops), except that z is
// the image itself: a training batch is small, and with n fixed per workgroup the nine operand offsets n * bs fold
// into the base pointers once (with a loop over n the backward kernel ran out of scalar registers).  A lane reads the
// byte and the pair of (n, p) once and keeps them in registers over the channels it walks; consecutive lanes on
// consecutive addresses in every operand; no position index is divided out of a flat one.
__global__ __launch_bounds__(256) void gc_qm_fwd_kernel(const GcQsDesc d, const unsigned char* __restrict__ qmap) {
  const int n = blockIdx.z;
  for (long long p = blockIdx.x * 256 + threadIdx.x; p < d.HW; p += gridDim.x * 256) {
    {
      const float2 si = d.steps[qmap[(long long)n * d.HW + p]];   // x: step, y: inv
      for (int c = blockIdx.y; c < d.C; c += gridDim.y) {
        const long long r = (long long)c * d.HW + p;
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
    }
  }
}

__global__ __launch_bounds__(256) void gc_qm_bwd_kernel(const GcQsBwdDesc d, const unsigned char* __restrict__ qmap) {
  const int n = blockIdx.z;
  for (long long p = blockIdx.x * 256 + threadIdx.x; p < d.HW; p += gridDim.x * 256) {
    {
      const float inv = d.steps[qmap[(long long)n * d.HW + p]].y;
      for (int c = blockIdx.y; c < d.C; c += gridDim.y) {
        const long long r = (long long)c * d.HW + p;
        const float y = d.y[n * d.y_bs + r], mu = d.mu[n * d.mu_bs + r], sc = d.sc[n * d.sc_bs + r];
        const float w = d.noise ? mul_rn(y - mu, inv) + d.noise[n * d.nz_bs + r] : (float)symbol_of(y, mu, inv);
        const float v = fabsf(w);
        const float se = mul_rn(fmaxf(sc, d.scale_bound), inv);
        const float u = (0.5f - v) / se, l = (-0.5f - v) / se;
        const float lraw = std_cdf(u) - std_cdf(l);
        float g = d.dlik[n * d.dl_bs + r];
        if (!(lraw >= d.lik_bound || g < 0.0f)) g = 0.0f;
        const float pu = std_pdf(u), pl = std_pdf(l);
        const float dv = g * (pl - pu) / se;
        float gs = g * (l * pl - u * pu) / se * inv;
        if (!(sc >= d.scale_bound || gs < 0.0f)) gs = 0.0f;
        const float sg = w > 0.0f ? 1.0f : (w < 0.0f ? -1.0f : 0.0f);
        float gy = 0.0f, gmu = 0.0f;
        if (d.noise) {
          gy = dv * sg * inv;
          gmu = -gy;
        }
        if (d.dyh) gy += d.dyh[n * d.dyh_bs + r];
        float* dyp = d.dy + n * d.dy_bs + r;
        if (d.accum_dy) gy += *dyp;
        *dyp = gy;
        d.dmu[n * d.dmu_bs + r] = gmu;
        d.dsc[n * d.dsc_bs + r] = gs;
      }
    }
  }
}

// ---- painting the training maps on the device: qmap [N][h][w] int8; every cell of image n holds base[n], then the R
// rectangles rects[n][r] = (y0, x0, y1, x1, k) (cells, half open) are painted in order, later ones winning
// (icm_amd/codec.py: roi_map).  One lane per cell walks the image's rectangles (R is small and the reads are
// wave-uniform) and stores once; a rectangle is clipped to the map by the test itself, an empty one holds no cell.
// grid (blocks over h * w, N); k and the coordinates are not range-checked.
__global__ __launch_bounds__(256) void qmap_paint_kernel(const signed char* __restrict__ base,
                                                          const int* __restrict__ rects, int R, int h, int w,
                                                          signed char* __restrict__ qmap) {
  const int n = blockIdx.y, hw = h * w;
  const int* rn = rects + (long long)n * R * 5;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < hw; p += gridDim.x * 256) {   // hw <= 2^30: no overflow
    const int cy = p / w, cx = p - cy * w;
    int k = base[n];
    for (int r = 0; r < R; ++r) {
      const int* q = rn + 5 * r;
      if (cy >= q[0] && cx >= q[1] && cy < q[2] && cx < q[3]) k = q[4];
    }
    qmap[(long long)n * hw + p] = (signed char)k;
  }
}

}  // namespace icm

using namespace icm;

static inline bool step_ok(float v) { return std::isfinite(v) && v > 0.0f; }
static inline bool dims_ok(int N, int C, int HW) { return N >= 1 && C >= 1 && HW >= 1; }
static inline int q_blocks(long long total) {
  return (int)std::max<long long>(1, std::min<long long>((total + 255) / 256, 256));
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

// grid of the map pair of the training step and of the RDOQ kernel: qmap_grid's x and y, and z = n (a grid's z holds
// 65 535)
constexpr int QM_MAX_N = 65535;
static inline dim3 qm_grid(int N, int C, int HW) {
  const dim3 g = qmap_grid(1, C, HW);
  return dim3(g.x, g.y, N);
}

extern "C" {

int icm_gc_code_q(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale, int64_t sc_bs,
                  const float* scale_table, int ns, float scale_bound, float step, float inv, int32_t* symbols,
                  int32_t* indexes, float* yh, int64_t yh_bs, int N, int C, int HW, void* stream) {
  if (!y || !mu || !scale || !scale_table || !symbols || !indexes || !yh) return ICM_ERR_ARG;
  if (!step_ok(step) || !step_ok(inv) || ns < 1 || !dims_ok(N, C, HW)) return ICM_ERR_ARG;
  const QGeom g{y_bs, mu_bs, sc_bs, yh_bs, N, C, HW};
  hipLaunchKernelGGL(gc_code_q_kernel, dim3(q_blocks((long long)N * C * HW)), dim3(256), 0, (hipStream_t)stream, y, mu,
                     scale, scale_table, ns, scale_bound, step, inv, symbols, indexes, yh, g);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_gc_indexes_q(const float* scale, int64_t sc_bs, const float* scale_table, int ns, float scale_bound, float inv,
                     int32_t* indexes, int N, int C, int HW, void* stream) {
  if (!scale || !scale_table || !indexes) return ICM_ERR_ARG;
  if (!step_ok(inv) || ns < 1 || !dims_ok(N, C, HW)) return ICM_ERR_ARG;
  const QGeom g{0, 0, sc_bs, 0, N, C, HW};
  hipLaunchKernelGGL(gc_indexes_q_kernel, dim3(q_blocks((long long)N * C * HW)), dim3(256), 0, (hipStream_t)stream,
                     scale, scale_table, ns, scale_bound, inv, indexes, g);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_dequantize_q(const int32_t* symbols, const float* mu, int64_t mu_bs, float step, float* yh, int64_t yh_bs, int N,
                     int C, int HW, void* stream) {
  if (!symbols || !mu || !yh) return ICM_ERR_ARG;
  if (!step_ok(step) || !dims_ok(N, C, HW)) return ICM_ERR_ARG;
  const QGeom g{0, mu_bs, 0, yh_bs, N, C, HW};
  hipLaunchKernelGGL(dequantize_q_kernel, dim3(q_blocks((long long)N * C * HW)), dim3(256), 0, (hipStream_t)stream,
                     symbols, mu, step, yh, g);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_gc_code_qmap(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale, int64_t sc_bs,
                     const float* scale_table, int ns, float scale_bound, const int8_t* qmap, const float* step_table,
                     int32_t* symbols, int32_t* indexes, float* yh, int64_t yh_bs, int N, int C, int HW, void* stream) {
  if (!y || !mu || !scale || !scale_table || !qmap || !step_table || !symbols || !indexes || !yh) return ICM_ERR_ARG;
  if (ns < 1 || !dims_ok(N, C, HW)) return ICM_ERR_ARG;
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
  if (!y || !mu || !scale || !scale_table || !symbols || !indexes || !yh) return ICM_ERR_ARG;
  if (!cdfs || !cdf_sizes || !offsets || !bits) return ICM_ERR_ARG;
  if ((qmap == nullptr) != (step_table == nullptr)) return ICM_ERR_ARG;
  if (!step_ok(step) || !step_ok(inv) || !step_ok(w) || !dims_ok(N, C, HW)) return ICM_ERR_ARG;
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
  if (!scale || !scale_table || !qmap || !step_table || !indexes) return ICM_ERR_ARG;
  if (ns < 1 || !dims_ok(N, C, HW)) return ICM_ERR_ARG;
  const QGeom g{0, 0, sc_bs, 0, N, C, HW};
  hipLaunchKernelGGL(gc_indexes_qmap_kernel, qmap_grid(N, C, HW), dim3(256), 0, (hipStream_t)stream, scale, scale_table,
                     ns, scale_bound, (const unsigned char*)qmap, (const float2*)step_table, indexes, g);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_dequantize_qmap(const int32_t* symbols, const float* mu, int64_t mu_bs, const int8_t* qmap,
                        const float* step_table, float* yh, int64_t yh_bs, int N, int C, int HW, void* stream) {
  if (!symbols || !mu || !qmap || !step_table || !yh) return ICM_ERR_ARG;
  if (!dims_ok(N, C, HW)) return ICM_ERR_ARG;
  const QGeom g{0, mu_bs, 0, yh_bs, N, C, HW};
  hipLaunchKernelGGL(dequantize_qmap_kernel, qmap_grid(N, C, HW), dim3(256), 0, (hipStream_t)stream, symbols, mu,
                     (const unsigned char*)qmap, (const float2*)step_table, yh, g);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

// the grid of icm_gc_likelihood_ste_fwd / _bwd: a training slice of a 16 x 256 x 256 batch has 131 072 elements
static inline int qs_blocks(long long total) {
  return (int)std::max<long long>(1, std::min<long long>((total + 255) / 256, 2048));
}

int icm_gc_likelihood_ste_qs_fwd(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale,
                                 int64_t sc_bs, const float* noise, int64_t nz_bs, const float* steps, float* lik,
                                 int64_t lik_bs, float* yh, int64_t yh_bs, float* yh2, int64_t yh2_bs, int N, int C,
                                 int HW, float scale_bound, float lik_bound, void* stream) {
  if (!y || !mu || !scale || !steps || !lik || N <= 0 || C <= 0 || HW <= 0 || scale_bound <= 0) return ICM_ERR_ARG;
  const GcQsDesc d{y, mu, scale, noise, (const float2*)steps, lik, yh, yh2, y_bs, mu_bs, sc_bs, nz_bs, lik_bs, yh_bs,
                   yh2_bs, N, C, HW, scale_bound, lik_bound};
  hipLaunchKernelGGL(gc_qs_fwd_kernel, dim3(qs_blocks((long long)N * C * HW)), dim3(256), 0, (hipStream_t)stream, d);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_gc_likelihood_ste_qs_bwd(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale,
                                 int64_t sc_bs, const float* noise, int64_t nz_bs, const float* steps, const float* dlik,
                                 int64_t dl_bs, const float* dyh, int64_t dyh_bs, float* dy, int64_t dy_bs, float* dmu,
                                 int64_t dmu_bs, float* dscale, int64_t dsc_bs, int N, int C, int HW, float scale_bound,
                                 float lik_bound, int accum_dy, void* stream) {
  if (!y || !mu || !scale || !steps || !dlik || !dy || !dmu || !dscale || N <= 0 || C <= 0 || HW <= 0)
    return ICM_ERR_ARG;
  const GcQsBwdDesc d{y, mu, scale, noise, (const float2*)steps, dlik, dyh, dy, dmu, dscale, y_bs, mu_bs, sc_bs, nz_bs,
                      dl_bs, dyh_bs, dy_bs, dmu_bs, dsc_bs, N, C, HW, accum_dy, scale_bound, lik_bound};
  hipLaunchKernelGGL(gc_qs_bwd_kernel, dim3(qs_blocks((long long)N * C * HW)), dim3(256), 0, (hipStream_t)stream, d);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_gc_likelihood_ste_qm_fwd(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale,
                                 int64_t sc_bs, const float* noise, int64_t nz_bs, const int8_t* qmap,
                                 const float* step_table, float* lik, int64_t lik_bs, float* yh, int64_t yh_bs,
                                 float* yh2, int64_t yh2_bs, int N, int C, int HW, float scale_bound, float lik_bound,
                                 void* stream) {
  if (!y || !mu || !scale || !qmap || !step_table || !lik || N <= 0 || C <= 0 || HW <= 0 || scale_bound <= 0 ||
      N > QM_MAX_N)
    return ICM_ERR_ARG;
  const GcQsDesc d{y, mu, scale, noise, (const float2*)step_table, lik, yh, yh2, y_bs, mu_bs, sc_bs, nz_bs, lik_bs,
                   yh_bs, yh2_bs, N, C, HW, scale_bound, lik_bound};
  hipLaunchKernelGGL(gc_qm_fwd_kernel, qm_grid(N, C, HW), dim3(256), 0, (hipStream_t)stream, d,
                     (const unsigned char*)qmap);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_gc_likelihood_ste_qm_bwd(const float* y, int64_t y_bs, const float* mu, int64_t mu_bs, const float* scale,
                                 int64_t sc_bs, const float* noise, int64_t nz_bs, const int8_t* qmap,
                                 const float* step_table, const float* dlik, int64_t dl_bs, const float* dyh,
                                 int64_t dyh_bs, float* dy, int64_t dy_bs, float* dmu, int64_t dmu_bs, float* dscale,
                                 int64_t dsc_bs, int N, int C, int HW, float scale_bound, float lik_bound, int accum_dy,
                                 void* stream) {
  if (!y || !mu || !scale || !qmap || !step_table || !dlik || !dy || !dmu || !dscale || N <= 0 || C <= 0 || HW <= 0 ||
      N > QM_MAX_N)
    return ICM_ERR_ARG;
  const GcQsBwdDesc d{y, mu, scale, noise, (const float2*)step_table, dlik, dyh, dy, dmu, dscale, y_bs, mu_bs, sc_bs,
                      nz_bs, dl_bs, dyh_bs, dy_bs, dmu_bs, dsc_bs, N, C, HW, accum_dy, scale_bound, lik_bound};
  hipLaunchKernelGGL(gc_qm_bwd_kernel, qm_grid(N, C, HW), dim3(256), 0, (hipStream_t)stream, d,
                     (const unsigned char*)qmap);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_qmap_paint(const int8_t* base, const int32_t* rects, int R, int8_t* qmap, int N, int h, int w, void* stream) {
  if (!base || !rects || !qmap || N < 1 || h < 1 || w < 1 || R < 0) return ICM_ERR_ARG;
  if ((long long)h * w > (1LL << 30) || N > 65535) return ICM_ERR_ARG;   // int cell indexes; N is the grid's y
  const int gx = (int)std::min<long long>(((long long)h * w + 255) / 256, 1024);
  hipLaunchKernelGGL(qmap_paint_kernel, dim3(gx, N), dim3(256), 0, (hipStream_t)stream, (const signed char*)base, rects,
                     R, h, w, (signed char*)qmap);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

}  // extern "C"
