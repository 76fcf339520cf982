// MS-SSIM (Wang, Simoncelli, Bovik 2003; the defaults of pytorch_msssim.ms_ssim) and its gradient with respect to the
// first image, f32, gfx950.  Plain vector code: the work is an 11-tap separable window over five products per pixel,
// i.e. LDS traffic and bandwidth; there is no contraction worth an MFMA.
//
// Forward, one launch per pyramid level (msssim_level_kernel): a workgroup owns a 32 x 32 tile of window statistics of
// one (n, c) plane.  It stages the 42 x 42 input pixels under that tile (tile + 10-pixel halo) of both images in LDS,
// filters the five products along the rows into LDS, along the columns out of LDS into registers, forms cs_map /
// ssim_map there, writes the three coefficient maps the backward needs, and leaves one (cs, ssim) partial sum per
// workgroup in the workspace.  The 2x2 average pooling that feeds the next level is done by the same workgroup from
// the staged tile.  The moments are those of the images minus data_range / 2: variances and covariances do not change
// under a shift, and E[xx] - mu^2 then cancels at the scale of the centred pixels instead of at mu^2 ~ data_range^2 / 4
// (in f32 that cancellation, compared with C2 on the smooth coarse levels, was the largest error of the whole value);
// the luminance term adds the shift back.  msssim_finish_kernel then adds the partials in tile order and forms
// ms[n, c], the mean and the per-level upstream factors w_l * ms / v_l (0 where v_l <= 0).  No float atomics anywhere:
// equal inputs give bit-identical results.
//
// Backward, one launch per level, last level first (msssim_bwd_level_kernel): the transpose of a valid filter is the
// full filter with the same (symmetric) window, so a workgroup that owns 32 x 32 INPUT pixels stages the 42 x 42
// coefficients above / left of them (zero outside the map, scaled by the plane's upstream factor), runs the same two
// passes over the three maps and combines   dX = a_f + 2 X b_f + Y c_f + pool_adjoint(dX of the next level).
#include "icm_common.h"

namespace {

constexpr int WIN = 11;            // window taps
constexpr int HALO = WIN - 1;      // 10
constexpr int T = 32;              // tile edge (statistics in the forward, input pixels in the backward)
constexpr int TIN = T + HALO;      // 42 staged rows / columns
constexpr int XS = 44;             // LDS row stride of a staged tile (multiple of 4: 16-byte row reads)
constexpr int LEVELS = 5;
constexpr int MIN_SIDE = HALO * 16;   // min(H, W) must exceed (11 - 1) * 2^4 = 160

struct Window {
  float g[WIN];
};

struct Plan {
  int h[LEVELS], w[LEVELS];          // level sizes
  int ty[LEVELS], tx[LEVELS];        // forward tiles per plane
  long long img[LEVELS];             // x pyramid of level l (l >= 1); the y pyramid follows it
  long long grad[LEVELS];            // gradient pyramid of level l (l >= 1)
  long long coef[LEVELS];            // 3 coefficient maps [3][NC][sh][sw]
  long long part[LEVELS];            // partial sums [NC][ty*tx][2], doubles
  long long lv, fac;                 // level values / upstream factors [5][NC]
  long long total;
};

inline long long al4(long long v) { return (v + 3) & ~3LL; }

bool make_plan(int N, int C, int H, int W, Plan& p) {
  if (N <= 0 || C <= 0 || H <= MIN_SIDE || W <= MIN_SIDE) return false;
  const long long NC = (long long)N * C;
  if (NC > 65535 || H > 32768 || W > 32768) return false;
  if (NC * H * W >= (1LL << 31)) return false;   // plane offsets are formed in 64 bits, pixel offsets in 32
  long long o = 0;
  p.h[0] = H;
  p.w[0] = W;
  for (int l = 0; l < LEVELS; ++l) {
    if (l) {
      p.h[l] = (p.h[l - 1] + 1) / 2;   // avg_pool2d(2, 2, padding = size % 2)
      p.w[l] = (p.w[l - 1] + 1) / 2;
    }
    const int sh = p.h[l] - HALO, sw = p.w[l] - HALO;
    p.ty[l] = (sh + T - 1) / T;
    p.tx[l] = (sw + T - 1) / T;
    p.img[l] = o;
    if (l) o += al4(2 * NC * p.h[l] * p.w[l]);
    p.grad[l] = o;
    if (l) o += al4(NC * p.h[l] * p.w[l]);
    p.coef[l] = o;
    o += al4(3 * NC * sh * sw);
    p.part[l] = o;
    o += al4(4 * NC * p.ty[l] * p.tx[l]);   // doubles
  }
  p.lv = o;
  o += al4(LEVELS * NC);
  p.fac = o;
  o += al4(LEVELS * NC);
  p.total = o;
  return true;
}

Window make_window() {
  Window wdw;
  double g[WIN], s = 0.0;
  for (int k = 0; k < WIN; ++k) {
    const double d = k - WIN / 2;
    g[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
    s += g[k];
  }
  for (int k = 0; k < WIN; ++k) wdw.g[k] = (float)(g[k] / s);
  return wdw;
}

// The map sums are carried in double from the per-thread sums on: a level value is a mean of up to ~10^5 maps close to
// 1, and an f32 tree would leave it with the few-ulp error that the finish then raises to a power and multiplies
// five times.  Fixed tree: lanes by xor butterfly, waves in index order.
__device__ __forceinline__ double block_sum_d(double v, double* red) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// stage rows [y0, y0 + TIN) x columns [x0, x0 + XS) of a h x w plane into dst[TIN][XS], zero outside the plane,
// every value times `scale`.  vec: w % 4 == 0, x0 % 4 == 0 and a 16-byte aligned plane (host-checked).
__device__ __forceinline__ void stage_tile(const float* __restrict__ src, int h, int w, int y0, int x0, float scale,
                                           int vec, float* dst) {
  if (vec) {
    for (int i = threadIdx.x; i < TIN * (XS / 4); i += 256) {
      const int r = i / (XS / 4), c = (i - r * (XS / 4)) * 4;
      const int y = y0 + r, x = x0 + c;
      f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
      if (y >= 0 && y < h && x >= 0 && x < w) v = *reinterpret_cast<const f32x4*>(src + (long long)y * w + x) * scale;
      *reinterpret_cast<f32x4*>(dst + r * XS + c) = v;
    }
  } else {
    for (int i = threadIdx.x; i < TIN * XS; i += 256) {
      const int r = i / XS, c = i - r * XS;
      const int y = y0 + r, x = x0 + c;
      float v = 0.0f;
      if (y >= 0 && y < h && x >= 0 && x < w) v = src[(long long)y * w + x] * scale;
      dst[r * XS + c] = v;
    }
  }
}

// 4 consecutive outputs of the 11-tap row filter from 14 inputs
__device__ __forceinline__ f32x4 row4(const float* v, const Window& wd) {
  f32x4 a = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < WIN; ++k) {
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = fmaf(wd.g[k], v[j + k], a[j]);
  }
  return a;
}
__device__ __forceinline__ void load16(const float* p, float* v) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p + 4 * q);
    v[4 * q] = t[0];
    v[4 * q + 1] = t[1];
    v[4 * q + 2] = t[2];
    v[4 * q + 3] = t[3];
  }
}
// 4 consecutive rows (r0 .. r0 + 3) of the 11-tap column filter of buf[TIN][T] at column c
__device__ __forceinline__ void col4(const float* buf, int r0, int c, const Window& wd, float* out) {
  float v[4 + HALO];
#pragma unroll
  for (int i = 0; i < 4 + HALO; ++i) v[i] = buf[(r0 + i) * T + c];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float a = 0.0f;
#pragma unroll
    for (int k = 0; k < WIN; ++k) a = fmaf(wd.g[k], v[j + k], a);
    out[j] = a;
  }
}

// pooled-row range owned by the tile whose first input row is t0: pooled row i reads rows 2i - pad and 2i - pad + 1
// and belongs to the tile that holds max(2i - pad, 0); the last tile also owns the rows under its halo
__device__ __forceinline__ void pool_range(int t0, int last, int pad, int n2, int& lo, int& hi) {
  lo = t0 == 0 ? 0 : (t0 + pad + 1) >> 1;
  hi = last ? n2 : (t0 + T + pad + 1) >> 1;
}

__global__ __launch_bounds__(256) void msssim_level_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                           int h, int w, float C1, float C2, float shift,
                                                           int last_level,
                                                           float* __restrict__ Xn, float* __restrict__ Yn,
                                                           float* __restrict__ coef, double* __restrict__ part, int vec,
                                                           const Window wd) {
  __shared__ __attribute__((aligned(16))) float xs[TIN * XS];
  __shared__ __attribute__((aligned(16))) float ys[TIN * XS];
  __shared__ __attribute__((aligned(16))) float hb[5][TIN * T];
  __shared__ double red[4];
  const int p = blockIdx.z, NC = gridDim.z;
  const int ty0 = blockIdx.y * T, tx0 = blockIdx.x * T;
  const int sh = h - HALO, sw = w - HALO;
  const long long plane = (long long)p * h * w;
  stage_tile(X + plane, h, w, ty0, tx0, 1.0f, vec, xs);
  stage_tile(Y + plane, h, w, ty0, tx0, 1.0f, vec, ys);
  __syncthreads();

  // rows: mu1, mu2, E[xx], E[yy], E[xy] of the centred images
  for (int it = threadIdx.x; it < TIN * (T / 4); it += 256) {
    const int r = it >> 3, c = (it & 7) * 4;
    float xv[16], yv[16], t[16];
    load16(xs + r * XS + c, xv);
    load16(ys + r * XS + c, yv);
#pragma unroll
    for (int i = 0; i < 14; ++i) {
      xv[i] -= shift;
      yv[i] -= shift;
    }
    *reinterpret_cast<f32x4*>(&hb[0][r * T + c]) = row4(xv, wd);
    *reinterpret_cast<f32x4*>(&hb[1][r * T + c]) = row4(yv, wd);
#pragma unroll
    for (int i = 0; i < 14; ++i) t[i] = xv[i] * xv[i];
    *reinterpret_cast<f32x4*>(&hb[2][r * T + c]) = row4(t, wd);
#pragma unroll
    for (int i = 0; i < 14; ++i) t[i] = yv[i] * yv[i];
    *reinterpret_cast<f32x4*>(&hb[3][r * T + c]) = row4(t, wd);
#pragma unroll
    for (int i = 0; i < 14; ++i) t[i] = xv[i] * yv[i];
    *reinterpret_cast<f32x4*>(&hb[4][r * T + c]) = row4(t, wd);
  }

  // 2x2 average pooling of the staged tile into the next level (zeros of the odd-size padding count in the /4)
  if (!last_level) {
    const int ph = h & 1, pw = w & 1, h2 = (h + 1) >> 1, w2 = (w + 1) >> 1;
    int ilo, ihi, jlo, jhi;
    pool_range(ty0, blockIdx.y == gridDim.y - 1, ph, h2, ilo, ihi);
    pool_range(tx0, blockIdx.x == gridDim.x - 1, pw, w2, jlo, jhi);
    const int nj = jhi - jlo, cnt = (ihi - ilo) * nj;
    const long long plane2 = (long long)p * h2 * w2;
    for (int k = threadIdx.x; k < cnt; k += 256) {
      const int i = ilo + k / nj, j = jlo + k % nj;
      const int r = 2 * i - ph - ty0, c = 2 * j - pw - tx0;   // -1 = the padded row / column
      float sx = 0.0f, sy = 0.0f;
#pragma unroll
      for (int dr = 0; dr < 2; ++dr) {
#pragma unroll
        for (int dc = 0; dc < 2; ++dc) {
          const int rr = r + dr, cc = c + dc;
          if (rr >= 0 && cc >= 0) {
            sx += xs[rr * XS + cc];
            sy += ys[rr * XS + cc];
          }
        }
      }
      Xn[plane2 + (long long)i * w2 + j] = 0.25f * sx;
      Yn[plane2 + (long long)i * w2 + j] = 0.25f * sy;
    }
  }
  __syncthreads();

  // columns, maps and coefficients: thread = column c, rows 4 rg .. 4 rg + 3
  const int c = threadIdx.x & 31, r0 = (threadIdx.x >> 5) * 4;
  float mu1[4], mu2[4], exx[4], eyy[4], exy[4];
  col4(hb[0], r0, c, wd, mu1);
  col4(hb[1], r0, c, wd, mu2);
  col4(hb[2], r0, c, wd, exx);
  col4(hb[3], r0, c, wd, eyy);
  col4(hb[4], r0, c, wd, exy);
  double cs_sum = 0.0, ss_sum = 0.0;
  const long long cmap = (long long)NC * sh * sw;
  float* cp = coef + (long long)p * sh * sw;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int sy = ty0 + r0 + j, sx = tx0 + c;
    if (sy < sh && sx < sw) {
      const float d1 = mu1[j], d2 = mu2[j];   // centred means
      const float s1 = exx[j] - d1 * d1, s2 = eyy[j] - d2 * d2, s12 = exy[j] - d1 * d2;
      const float m1 = d1 + shift, m2 = d2 + shift;
      const float rB2 = 1.0f / (s1 + s2 + C2), rB1 = 1.0f / (m1 * m1 + m2 * m2 + C1);
      const float cs = (2.0f * s12 + C2) * rB2;
      const float lum = (2.0f * m1 * m2 + C1) * rB1;
      cs_sum += (double)cs;
      ss_sum += (double)(lum * cs);
      // derivatives of the level's map with respect to mu1 (a), g*(X*X) (b), g*(X*Y) (c) of the images as given
      float a = 2.0f * (cs * m1 - m2) * rB2, b = -cs * rB2, cc = 2.0f * rB2;
      if (last_level) {
        a = lum * a + cs * 2.0f * (m2 - m1 * lum) * rB1;
        b *= lum;
        cc *= lum;
      }
      const long long o = (long long)sy * sw + sx;
      cp[o] = a;
      cp[cmap + o] = b;
      cp[2 * cmap + o] = cc;
    }
  }
  cs_sum = block_sum_d(cs_sum, red);
  ss_sum = block_sum_d(ss_sum, red);
  if (threadIdx.x == 0) {
    const long long o = 2 * ((long long)p * gridDim.y * gridDim.x + blockIdx.y * gridDim.x + blockIdx.x);
    part[o] = cs_sum;
    part[o + 1] = ss_sum;
  }
}

struct FinishArgs {
  long long part[LEVELS];   // float offset of the level's partials in ws (doubles, 16-byte aligned)
  int tiles[LEVELS];
  double inv_count[LEVELS];
};

// one workgroup: thread t takes planes t, t + 256, ...; partials are added in tile order.  Double throughout (a few
// hundred operations per plane): what reaches f32 is rounded once.
__global__ __launch_bounds__(256) void msssim_finish_kernel(const float* __restrict__ ws, const FinishArgs fa, int NC,
                                                            float* __restrict__ lv, float* __restrict__ fac,
                                                            float* __restrict__ ms, float* __restrict__ out,
                                                            float lmbda, float* __restrict__ loss_io) {
  __shared__ double red[4];
  const double wl[LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
  double acc = 0.0;
  for (int p = threadIdx.x; p < NC; p += 256) {
    double v[LEVELS], prod = 1.0;
#pragma unroll
    for (int l = 0; l < LEVELS; ++l) {
      const double* q = reinterpret_cast<const double*>(ws + fa.part[l]) + 2LL * p * fa.tiles[l] + (l == LEVELS - 1 ? 1 : 0);
      double s = 0.0;
      for (int t = 0; t < fa.tiles[l]; ++t) s += q[2 * t];
      v[l] = fmax(s * fa.inv_count[l], 0.0);   // relu
      lv[l * NC + p] = (float)v[l];
      prod *= v[l] > 0.0 ? pow(v[l], wl[l]) : 0.0;
    }
    ms[p] = (float)prod;
    acc += prod;
#pragma unroll
    for (int l = 0; l < LEVELS; ++l) fac[l * NC + p] = v[l] > 0.0 ? (float)(wl[l] * prod / v[l]) : 0.0f;
  }
  acc = block_sum_d(acc, red);
  if (threadIdx.x == 0) {
    const double mean = acc / (double)NC;
    out[0] = (float)mean;
    out[1] = (float)(1.0 - mean);
    if (loss_io) *loss_io += (float)((double)lmbda * (1.0 - mean));
  }
}

__global__ __launch_bounds__(256) void msssim_bwd_level_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                               int h, int w, const float* __restrict__ coef,
                                                               const float* __restrict__ fac,
                                                               const float* __restrict__ gplane, float gscale,
                                                               const float* __restrict__ gnext, float* __restrict__ dX,
                                                               const Window wd) {
  __shared__ __attribute__((aligned(16))) float ms_[3][TIN * XS];
  __shared__ __attribute__((aligned(16))) float hb[3][TIN * T];
  const int p = blockIdx.z, NC = gridDim.z;
  const int ty0 = blockIdx.y * T, tx0 = blockIdx.x * T;
  const int sh = h - HALO, sw = w - HALO;
  // upstream factor of this plane's level value, spread over the sh x sw means
  const float up = gplane ? gplane[p] * gscale : gscale / (float)NC;
  const float scale = fac[p] * up / (float)(sh * sw);
  const long long cmap = (long long)NC * sh * sw;
  const float* cp = coef + (long long)p * sh * sw;
#pragma unroll
  for (int q = 0; q < 3; ++q) stage_tile(cp + q * cmap, sh, sw, ty0 - HALO, tx0 - HALO, scale, 0, ms_[q]);
  __syncthreads();
  for (int it = threadIdx.x; it < TIN * (T / 4); it += 256) {
    const int r = it >> 3, c = (it & 7) * 4;
    float v[16];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      load16(ms_[q] + r * XS + c, v);
      *reinterpret_cast<f32x4*>(&hb[q][r * T + c]) = row4(v, wd);
    }
  }
  __syncthreads();
  const int c = threadIdx.x & 31, r0 = (threadIdx.x >> 5) * 4;
  float af[4], bf[4], cf[4];
  col4(hb[0], r0, c, wd, af);
  col4(hb[1], r0, c, wd, bf);
  col4(hb[2], r0, c, wd, cf);
  const int x = tx0 + c;
  const int ph = h & 1, pw = w & 1, w2 = (w + 1) >> 1, h2 = (h + 1) >> 1;
  const long long plane = (long long)p * h * w;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int y = ty0 + r0 + j;
    if (y < h && x < w) {
      const long long o = plane + (long long)y * w + x;
      float g = af[j] + 2.0f * X[o] * bf[j] + Y[o] * cf[j];
      if (gnext) g += 0.25f * gnext[(long long)p * h2 * w2 + (long long)((y + ph) >> 1) * w2 + ((x + pw) >> 1)];
      dX[o] = g;
    }
  }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" {

int64_t icm_msssim_workspace_floats(int N, int C, int H, int W) {
  Plan p;
  return make_plan(N, C, H, W, p) ? (int64_t)p.total : 0;
}

int icm_msssim_fwd(const float* x, const float* y, int N, int C, int H, int W, float data_range, float* ms, float* out,
                   float lmbda, float* loss_io, float* ws, int64_t ws_floats, void* stream) {
  Plan p;
  if (!x || !y || !ms || !out || !ws || !(data_range > 0.0f)) return ICM_ERR_ARG;
  if (!make_plan(N, C, H, W, p)) return ICM_ERR_ARG;
  if (ws_floats < p.total || (reinterpret_cast<uintptr_t>(ws) & 15)) return ICM_ERR_ARG;
  const int NC = N * C;
  const Window wd = make_window();
  const float C1 = (0.01f * data_range) * (0.01f * data_range), C2 = (0.03f * data_range) * (0.03f * data_range);
  FinishArgs fa;
  for (int l = 0; l < LEVELS; ++l) {
    const float* xl = l ? ws + p.img[l] : x;
    const float* yl = l ? ws + p.img[l] + (long long)NC * p.h[l] * p.w[l] : y;
    const int last = l == LEVELS - 1;
    float* xn = last ? nullptr : ws + p.img[l + 1];
    float* yn = last ? nullptr : xn + (long long)NC * p.h[l + 1] * p.w[l + 1];
    const int vec = (p.w[l] % 4 == 0) && ((reinterpret_cast<uintptr_t>(xl) | reinterpret_cast<uintptr_t>(yl)) & 15) == 0 &&
                    ((long long)p.h[l] * p.w[l]) % 4 == 0;
    hipLaunchKernelGGL(msssim_level_kernel, dim3(p.tx[l], p.ty[l], NC), dim3(256), 0, ST, xl, yl, p.h[l], p.w[l], C1, C2,
                       0.5f * data_range, last, xn, yn, ws + p.coef[l], reinterpret_cast<double*>(ws + p.part[l]), vec, wd);
    ICM_CHECK_LAUNCH();
    fa.part[l] = p.part[l];
    fa.tiles[l] = p.ty[l] * p.tx[l];
    fa.inv_count[l] = 1.0 / (double)((long long)(p.h[l] - HALO) * (p.w[l] - HALO));
  }
  hipLaunchKernelGGL(msssim_finish_kernel, dim3(1), dim3(256), 0, ST, ws, fa, NC, ws + p.lv, ws + p.fac, ms, out, lmbda,
                     loss_io);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_msssim_bwd(const float* x, const float* y, int N, int C, int H, int W, const float* gplane, float gscale,
                   float* dx, float* ws, int64_t ws_floats, void* stream) {
  Plan p;
  if (!x || !y || !dx || !ws) return ICM_ERR_ARG;
  if (!make_plan(N, C, H, W, p)) return ICM_ERR_ARG;
  if (ws_floats < p.total) return ICM_ERR_ARG;
  const int NC = N * C;
  const Window wd = make_window();
  for (int l = LEVELS - 1; l >= 0; --l) {
    const float* xl = l ? ws + p.img[l] : x;
    const float* yl = l ? ws + p.img[l] + (long long)NC * p.h[l] * p.w[l] : y;
    const float* gnext = l == LEVELS - 1 ? nullptr : ws + p.grad[l + 1];
    float* dxl = l ? ws + p.grad[l] : dx;
    hipLaunchKernelGGL(msssim_bwd_level_kernel, dim3((p.w[l] + T - 1) / T, (p.h[l] + T - 1) / T, NC), dim3(256), 0, ST,
                       xl, yl, p.h[l], p.w[l], ws + p.coef[l], ws + p.fac + (long long)l * NC, gplane, gscale, gnext, dxl,
                       wd);
    ICM_CHECK_LAUNCH();
  }
  return ICM_OK;
}

}  // extern "C"
