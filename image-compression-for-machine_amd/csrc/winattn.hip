// Window multi-head self-attention core (forward + backward) on NCHW tensors, gfx950.
//
// Replaces WinBasedAttention / WindowAttention between the qkv and proj Linears
// (layers/win_attention.py:84-115,153-207).  The reference materialises six permuted copies
// (NCHW->NHWC, roll, window_partition, qkv reshape/permute, window_reverse, roll back, NHWC->NCHW);
// here the cyclic shift, window partition, head split, relative-position-bias gather and the 0/-100
// shift mask are pure address arithmetic on the NCHW qkv tensor produced by the 1x1-conv GEMM.
//
// One workgroup = one window of one image; each wave walks heads.  Lane = query token.  K and V of the
// head live in LDS (broadcast reads), the score row lives in a per-wave LDS matrix with odd row stride
// (conflict-free row and column sweeps), so the backward pass gets P^T / dS^T for dV, dK without any
// cross-lane shuffles.  Relative-position-bias gradients are reduced per wave in LDS (all lanes of one
// instruction hit distinct table entries); every (window, head) writes its partial table to a workspace slab
// and two small kernels add the slabs in window order: bitwise reproducible, no float atomics.
//
// Host side: fill_desc (winattn_common.h) checks the geometry, winattn_route walks the family table (matrix cores 8x8,
// matrix cores 4x4, the VALU kernels of this file) for the first family whose plan takes it, launch() starts the
// planned kernel; icm_winattn_fwd, icm_winattn_bwd and icm_debug_winattn_route are those three steps.
#include <algorithm>
#include "winattn_common.h"

namespace icm {

static int g_force_valu = 0;   // test hook: 1 = always take the generic (VALU) kernels below

// s = sum_d a[d] * row[d]; row is an LDS row shared by all lanes (broadcast): 16-byte reads when HD % 4 == 0
template <int HD>
__device__ __forceinline__ float dot_row(const float (&a)[HD], const float* __restrict__ row) {
  float s = 0.0f;
  if constexpr (HD % 4 == 0) {
    const f32x4* r4 = reinterpret_cast<const f32x4*>(row);
#pragma unroll
    for (int q = 0; q < HD / 4; ++q) {
      const f32x4 v = r4[q];
      s += a[4 * q] * v[0];
      s += a[4 * q + 1] * v[1];
      s += a[4 * q + 2] * v[2];
      s += a[4 * q + 3] * v[3];
    }
  } else {
#pragma unroll
    for (int dd = 0; dd < HD; ++dd) s += a[dd] * row[dd];
  }
  return s;
}
// o[d] += p * row[d]
template <int HD>
__device__ __forceinline__ void axpy_row(float (&o)[HD], float p, const float* __restrict__ row) {
  if constexpr (HD % 4 == 0) {
    const f32x4* r4 = reinterpret_cast<const f32x4*>(row);
#pragma unroll
    for (int q = 0; q < HD / 4; ++q) {
      const f32x4 v = r4[q];
      o[4 * q] += p * v[0];
      o[4 * q + 1] += p * v[1];
      o[4 * q + 2] += p * v[2];
      o[4 * q + 3] += p * v[3];
    }
  } else {
#pragma unroll
    for (int dd = 0; dd < HD; ++dd) o[dd] += p * row[dd];
  }
}

template <int HD>
__global__ __launch_bounds__(256) void winattn_fwd_kernel(const WaDesc d) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane64 = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
  const int T = d.T, TS = T + 1;
  // small windows (T = 16): G = 64 / T heads share a wave, lane = (head group, token)
  const int G = d.G, grp = lane64 / T, lane = lane64 - grp * T;
  float* Ksh = smem + (wave * G + grp) * (2 * T * HD + T * TS);
  float* Vsh = Ksh + T * HD;
  float* Ssh = Vsh + T * HD;
  // XCD-aware window order: horizontally adjacent windows (which share every 128-B line of a 4- or 8-pixel-wide row
  // segment) meet in one L2
  int bid = xcd_block_id();
  const int wx = bid % d.nwx; bid /= d.nwx;
  const int wy = bid % d.nwy;
  const int n = bid / d.nwy;
  const long long HW = (long long)d.H * d.W;
  const float* base = d.qkv + (long long)n * 3 * d.C * HW;
  const Tok me = token(d, d.ws, wy, wx, lane);
  const int tw = 2 * d.ws - 1;

  for (int head0 = wave * G; head0 < d.heads; head0 += nwaves * G) {
    const int head = min(head0 + grp, d.heads - 1);
    const bool active = grp < G && head0 + grp < d.heads;
    const float* qp = base + (long long)(head * HD) * HW;
    const float* kp = base + (long long)(d.C + head * HD) * HW;
    const float* vp = base + (long long)(2 * d.C + head * HD) * HW;
    float q[HD];
    if (active) {
#pragma unroll
      for (int dd = 0; dd < HD; ++dd) {
        q[dd] = qp[dd * HW + me.pix] * d.scale;
        Ksh[lane * HD + dd] = kp[dd * HW + me.pix];
        Vsh[lane * HD + dd] = vp[dd * HW + me.pix];
      }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    float m = -3.0e38f;
    if (active) {
      for (int j = 0; j < T; ++j) {
        float s = dot_row<HD>(q, Ksh + j * HD);
        const Tok tj = token(d, d.ws, wy, wx, j);
        const int idx = (me.r - tj.r + d.ws - 1) * tw + (me.c - tj.c + d.ws - 1);
        s += d.table[idx * d.heads + head];
        if (d.shift > 0 && tj.lab != me.lab) s += -100.0f;
        Ssh[lane * TS + j] = s;
        m = fmaxf(m, s);
      }
      float l = 0.0f;
      for (int j = 0; j < T; ++j) {
        const float p = expf(Ssh[lane * TS + j] - m);
        Ssh[lane * TS + j] = p;
        l += p;
      }
      const float inv = 1.0f / l;
      float o[HD];
#pragma unroll
      for (int dd = 0; dd < HD; ++dd) o[dd] = 0.0f;
      for (int j = 0; j < T; ++j) {
        const float p = Ssh[lane * TS + j] * inv;
        axpy_row<HD>(o, p, Vsh + j * HD);
      }
      float* op = d.out + ((long long)n * d.C + head * HD) * HW;
#pragma unroll
      for (int dd = 0; dd < HD; ++dd) op[dd * HW + me.pix] = o[dd];
    }
    __builtin_amdgcn_wave_barrier();
  }
}

template <int HD>
__global__ __launch_bounds__(128) void winattn_bwd_kernel(const WaDesc d) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane64 = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
  const int T = d.T, TS = T + 1;
  const int tw = 2 * d.ws - 1, ntab = tw * tw;
  // LDS per head: K | V | dO | S.  Two regions are recycled so that two workgroups fit one CU (35 KB per head for
  // 8x8 windows): dO is dead after dV -> it becomes the per-head table-gradient accumulator; V is dead after
  // dP / dq -> the scaled q (kept in registers until then) is parked there for dK.
  const int per_wave = (3 * T * HD + T * TS + 3) & ~3;   // keep every slab 16-B aligned (b128 reads)
  const int G = d.G, grp = lane64 / T, lane = lane64 - grp * T;     // G heads per wave for small windows
  float* Ksh = smem + (wave * G + grp) * per_wave;
  float* Vsh = Ksh + T * HD;
  float* Gsh = Vsh + T * HD;   // dO
  float* Ssh = Gsh + T * HD;   // P then dS
  float* Qsh = Vsh;            // scaled q, written after the dq phase
  float* Bsh = Gsh;            // per-head table gradient, zeroed after the dV phase
  // XCD-aware window order: horizontally adjacent windows (which share every 128-B line of a 4- or 8-pixel-wide row
  // segment) meet in one L2
  int bid = xcd_block_id();
  const int win = bid;
  const int wx = bid % d.nwx; bid /= d.nwx;
  const int wy = bid % d.nwy;
  const int n = bid / d.nwy;
  const long long HW = (long long)d.H * d.W;
  const float* base = d.qkv + (long long)n * 3 * d.C * HW;
  float* dbase = d.dqkv + (long long)n * 3 * d.C * HW;
  const Tok me = token(d, d.ws, wy, wx, lane);

  for (int head0 = wave * G; head0 < d.heads; head0 += nwaves * G) {
    const int head = min(head0 + grp, d.heads - 1);
    const bool active = grp < G && head0 + grp < d.heads;
    const float* qp = base + (long long)(head * HD) * HW;
    const float* kp = base + (long long)(d.C + head * HD) * HW;
    const float* vp = base + (long long)(2 * d.C + head * HD) * HW;
    const float* gp = d.dout + ((long long)n * d.C + head * HD) * HW;
    float q[HD], go[HD];
    if (active) {
#pragma unroll
      for (int dd = 0; dd < HD; ++dd) {
        q[dd] = qp[dd * HW + me.pix] * d.scale;
        go[dd] = gp[dd * HW + me.pix];
        Gsh[lane * HD + dd] = go[dd];
        Ksh[lane * HD + dd] = kp[dd * HW + me.pix];
        Vsh[lane * HD + dd] = vp[dd * HW + me.pix];
      }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    // ---- recompute P (row per lane)
    float inv = 0.0f;
    if (active) {
      float m = -3.0e38f;
      for (int j = 0; j < T; ++j) {
        float s = dot_row<HD>(q, Ksh + j * HD);
        const Tok tj = token(d, d.ws, wy, wx, j);
        const int idx = (me.r - tj.r + d.ws - 1) * tw + (me.c - tj.c + d.ws - 1);
        s += d.table[idx * d.heads + head];
        if (d.shift > 0 && tj.lab != me.lab) s += -100.0f;
        Ssh[lane * TS + j] = s;
        m = fmaxf(m, s);
      }
      float l = 0.0f;
      for (int j = 0; j < T; ++j) {
        const float p = expf(Ssh[lane * TS + j] - m);
        Ssh[lane * TS + j] = p;
        l += p;
      }
      inv = 1.0f / l;
      for (int j = 0; j < T; ++j) Ssh[lane * TS + j] *= inv;
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    // ---- dV[j][:] = sum_i P[i][j] dO[i][:]   (lane = j, column sweep of P)
    if (active) {
      float acc[HD];
#pragma unroll
      for (int dd = 0; dd < HD; ++dd) acc[dd] = 0.0f;
      for (int i = 0; i < T; ++i) {
        const float p = Ssh[i * TS + lane];
        axpy_row<HD>(acc, p, Gsh + i * HD);
      }
      float* dv = dbase + (long long)(2 * d.C + head * HD) * HW;
#pragma unroll
      for (int dd = 0; dd < HD; ++dd) dv[dd * HW + me.pix] = acc[dd];
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    if (grp < G)   // dO rows are dead: the region now accumulates the table gradient
      for (int i = lane; i < ntab; i += T) Bsh[i] = 0.0f;
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    // ---- dP, delta, dS (row per lane), dq, table gradient
    if (active) {
      float delta = 0.0f;
      for (int j = 0; j < T; ++j) {
        const float dp = dot_row<HD>(go, Vsh + j * HD);
        delta += Ssh[lane * TS + j] * dp;
      }
      float dq[HD];
#pragma unroll
      for (int dd = 0; dd < HD; ++dd) dq[dd] = 0.0f;
      for (int j = 0; j < T; ++j) {
        const float dp = dot_row<HD>(go, Vsh + j * HD);
        const float ds = Ssh[lane * TS + j] * (dp - delta);
        Ssh[lane * TS + j] = ds;
        axpy_row<HD>(dq, ds, Ksh + j * HD);
        const Tok tj = token(d, d.ws, wy, wx, j);
        const int idx = (me.r - tj.r + d.ws - 1) * tw + (me.c - tj.c + d.ws - 1);
        Bsh[idx] += ds;  // distinct idx across the active lanes of this instruction
      }
      float* dqp = dbase + (long long)(head * HD) * HW;
#pragma unroll
      for (int dd = 0; dd < HD; ++dd) dqp[dd * HW + me.pix] = dq[dd] * d.scale;
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    if (active) {   // V rows are dead: park the scaled q there for the dK sweep
#pragma unroll
      for (int dd = 0; dd < HD; ++dd) Qsh[lane * HD + dd] = q[dd];
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    // ---- dK[j][:] = sum_i dS[i][j] q[i][:]   (lane = j)
    if (active) {
      float acc[HD];
#pragma unroll
      for (int dd = 0; dd < HD; ++dd) acc[dd] = 0.0f;
      for (int i = 0; i < T; ++i) {
        const float ds = Ssh[i * TS + lane];
        axpy_row<HD>(acc, ds, Qsh + i * HD);
      }
      float* dk = dbase + (long long)(d.C + head * HD) * HW;
#pragma unroll
      for (int dd = 0; dd < HD; ++dd) dk[dd * HW + me.pix] = acc[dd];
    }
    if (active) {
      float* slab = d.dtable_ws + ((long long)win * d.heads + head) * ntab;
      for (int i = lane; i < ntab; i += T) slab[i] = Bsh[i];
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
  }
}

// Table-gradient reduction, stage 1: part[s][e] = sum over the windows of chunk s of slab[w][e], e = head*ntab + i.
// Workgroup = 64 entries x 4 window lanes; window lanes are combined in lane order through LDS.
__global__ __launch_bounds__(256) void dtable_reduce1_kernel(const float* __restrict__ slabs, float* __restrict__ part,
                                                             int E, int nwin, int chunk) {
  __shared__ float red[4][64];
  const int e = blockIdx.x * 64 + (threadIdx.x & 63), wl = threadIdx.x >> 6, s = blockIdx.y;
  const int w0 = s * chunk, w1 = min(nwin, w0 + chunk);
  float acc = 0.0f;
  if (e < E)
    for (int w = w0 + wl; w < w1; w += 4) acc += slabs[(long long)w * E + e];
  red[wl][threadIdx.x & 63] = acc;
  __syncthreads();
  if (wl == 0 && e < E)
    part[(long long)s * E + e] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
// stage 2: dtable[i*heads + head] (+)= sum_s part[s][head*ntab + i]
__global__ void dtable_reduce2_kernel(const float* __restrict__ part, float* __restrict__ dtable, int E, int S,
                                      int ntab, int heads, int accum) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  float acc = 0.0f;
  for (int s = 0; s < S; ++s) acc += part[(long long)s * E + e];
  const int head = e / ntab, i = e - head * ntab;
  float* o = dtable + i * heads + head;
  *o = accum ? *o + acc : acc;
}


static bool pick(int hd, int backward, void (*&fn)(const WaDesc)) {
  switch (hd) {
#define C_(n) case n: fn = backward ? winattn_bwd_kernel<n> : winattn_fwd_kernel<n>; return true;
    C_(8) C_(10) C_(16) C_(24) C_(32) C_(40) C_(48)
#undef C_
    default: return false;
  }
}

// the generic kernels: every window size fill_desc admits, one workgroup per window
static int valu_plan(const WaDesc& d, int backward, WaPlan& p) {
  if (!pick(d.hd, backward, p.fn)) return ICM_ERR_UNSUPPORTED;
  const int tw = 2 * d.ws - 1, wave_tasks = (d.heads + d.G - 1) / d.G;
  int waves;
  if (!backward) {
    waves = std::min(4, wave_tasks);
    p.lds = (size_t)waves * d.G * (2 * d.T * d.hd + d.T * (d.T + 1)) * 4;
  } else {
    if (tw * tw > d.T * d.hd) return ICM_ERR_UNSUPPORTED;   // the table gradient is accumulated in the dO region
    waves = std::min(2, wave_tasks);
    p.lds = (size_t)waves * d.G * ((3 * d.T * d.hd + d.T * (d.T + 1) + 3) & ~3) * 4;
  }
  p.grid = p.slabs = d.N * d.nwy * d.nwx;
  p.block = 64 * waves;
  return p.lds > kWaLdsLimit ? ICM_ERR_UNSUPPORTED : ICM_OK;
}

// The kernel families in trial order; the route code is what icm_debug_winattn_route reports.
enum { WA_ROUTE_VALU = 0, WA_ROUTE_MFMA = 1, WA_ROUTE_MFMA16 = 2 };
static const struct {
  int route;
  WaPlanFn plan;
} kWaFamilies[] = {{WA_ROUTE_MFMA, winattn_mfma_plan}, {WA_ROUTE_MFMA16, winattn_mfma16_plan}, {WA_ROUTE_VALU, valu_plan}};

// Which family serves a checked geometry (route) and how (p), or the code the call returns without launching: that of
// the last family tried.  The one decision behind icm_winattn_fwd, icm_winattn_bwd and icm_debug_winattn_route; no
// HIP call.
static int winattn_route(const WaDesc& d, int backward, int& route, WaPlan& p) {
  int rc = ICM_ERR_UNSUPPORTED;
  for (const auto& f : kWaFamilies) {
    if (g_force_valu && f.route != WA_ROUTE_VALU) continue;
    route = f.route;
    rc = f.plan(d, backward, p);
    if (rc == ICM_OK) break;
  }
  return rc;
}

// the only launch site of the attention kernels
static int launch(const WaDesc& d, const WaPlan& p, hipStream_t stream) {
  if (p.lds > 64 * 1024 && !ensure_max_lds(reinterpret_cast<const void*>(p.fn))) return ICM_ERR_LAUNCH;
  hipLaunchKernelGGL(p.fn, dim3(p.grid), dim3(p.block), p.lds, stream, d);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

// reduction plan of nslab table-gradient slabs: S partial sums over chunks of `chunk` slabs, S <= 64
static void dtable_chunks(int nslab, int& S, int& chunk) {
  S = std::max(1, std::min(64, nslab / 16));
  chunk = (nslab + S - 1) / S;
  S = (nslab + chunk - 1) / chunk;
}

}  // namespace icm

using namespace icm;
extern "C" {

void icm_debug_force_winattn_valu(int on) { icm::g_force_valu = on ? 1 : 0; }

int icm_debug_winattn_route(int N, int C, int H, int W, int heads, int ws, int shift, int backward) {
  WaDesc d{};
  int rc = fill_desc(d, N, C, H, W, heads, ws, shift);
  if (rc) return -rc;
  int route;
  WaPlan p;
  rc = winattn_route(d, backward ? 1 : 0, route, p);
  return rc ? -rc : route;
}

int icm_winattn_fwd(const float* qkv, const float* table, float* out, int N, int C, int H, int W, int heads, int ws,
                    int shift, void* stream) {
  if (!qkv || !table || !out) return ICM_ERR_ARG;
  WaDesc d{};
  int rc = fill_desc(d, N, C, H, W, heads, ws, shift);
  if (rc) return rc;
  int route;
  WaPlan p;
  rc = winattn_route(d, 0, route, p);
  if (rc) return rc;
  d.qkv = qkv; d.table = table; d.out = out;
  return launch(d, p, (hipStream_t)stream);
}

// one slab per window (the 4x4 matrix-core kernels write fewer: callers size for any family) + the S partial sums
int64_t icm_winattn_bwd_workspace_floats(int N, int C, int H, int W, int heads, int ws) {
  if (N <= 0 || heads <= 0 || ws <= 0 || H % ws || W % ws) return -1;
  const int tw = 2 * ws - 1, nwin = N * (H / ws) * (W / ws), E = heads * tw * tw;
  int S, chunk;
  dtable_chunks(nwin, S, chunk);
  return (int64_t)nwin * E + (int64_t)S * E;
}

int icm_winattn_bwd(const float* qkv, const float* table, const float* dout, float* dqkv, float* dtable,
                    int accum_table, float* wsp, int64_t ws_floats, int N, int C, int H, int W, int heads, int ws,
                    int shift, void* stream) {
  if (!qkv || !table || !dout || !dqkv || !dtable || !wsp) return ICM_ERR_ARG;
  WaDesc d{};
  int rc = fill_desc(d, N, C, H, W, heads, ws, shift);
  if (rc) return rc;
  if (ws_floats < icm_winattn_bwd_workspace_floats(N, C, H, W, heads, ws)) return ICM_ERR_ARG;
  int route;
  WaPlan p;
  rc = winattn_route(d, 1, route, p);
  if (rc) return rc;
  d.qkv = qkv; d.table = table; d.dout = dout; d.dqkv = dqkv; d.dtable_ws = wsp;
  rc = launch(d, p, (hipStream_t)stream);
  if (rc) return rc;
  const int tw = 2 * ws - 1, E = heads * tw * tw;
  int S, chunk;
  dtable_chunks(p.slabs, S, chunk);
  float* part = wsp + (long long)p.slabs * E;
  hipLaunchKernelGGL(dtable_reduce1_kernel, dim3((E + 63) / 64, S), dim3(256), 0, (hipStream_t)stream, wsp, part, E,
                     p.slabs, chunk);
  ICM_CHECK_LAUNCH();
  hipLaunchKernelGGL(dtable_reduce2_kernel, dim3((E + 255) / 256), dim3(256), 0, (hipStream_t)stream, part, dtable, E, S,
                     tw * tw, heads, accum_table);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

}  // extern "C"
