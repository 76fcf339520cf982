// Implicit-GEMM convolution family on f32 MFMA (v_mfma_f32_32x32x2_f32) for gfx950.
//
// One kernel serves conv fwd, conv dgrad, convT fwd, convT dgrad, 1x1 convs / Linear layers and the
// GDN channel contraction (reference call sites: include/icm_hip.h).  GEMM view per launch:
//     D[co][pixel] = sum_{tap, ci} Wp[tap][ci][co] * patch[ci][pixel + tap]
//   * M = output channels (MFMA A operand, rows), N = pixels (MFMA B operand, columns) so that the
//     32 lanes of a half-wave hold 32 consecutive pixels of one channel plane: NCHW loads and stores
//     are 128-B coalesced with no transposes anywhere;
//   * the input patch of the block's pixel tile (8 input channels per K-chunk, halo included) is
//     staged once into LDS and re-read for every tap (25x reuse for 5x5) -- activations are never
//     im2col-expanded in HBM or L2; stride-2 patches are stored column-parity-split so the B-fragment
//     ds_read_b32 is bank-conflict free;
//   * weights are pre-packed in MFMA A-fragment order (icm_pack_weights) and stream straight from
//     L2 into registers as one coalesced 16-B load per lane per (tap, 8-channel chunk, 32-co tile);
//   * "scatter" forms (convT fwd / conv dgrad) run as stride^2 output-parity classes, each a dense
//     stride-1 gather with its own tap subset -- no zero-stuffing, no atomics;
//   * pointwise neighbours are fused: operand activation on the LDS staging path (virtual GELU,
//     x^2 for GDN) and the epilogues listed in icm_hip.h (bias, residual, GDN rsqrt, GELU', LRP tanh,
//     PixelShuffle store, gradient accumulation), defined once for all conv kernels in conv_common.h.
#include <climits>
#include <cstdlib>
#include <vector>
#include "conv_common.h"

namespace icm {

// 512 threads: waves 0-3 issue MFMAs only (B fragments from LDS, A fragments = packed weights from L2);
// waves 4-7 are loaders that stage the NEXT K-chunk's halo patch into the other LDS buffer meanwhile.
// MFMA and VALU/VMEM are separate pipes per SIMD, so with one MFMA wave and one loader wave per SIMD the
// staging cost disappears behind the 64-cycle v_mfma_f32_32x32x2_f32 issue interval.
// KS > 1: intra-workgroup split-K for small problems (few output tiles, deep K): KS MFMA waves share one output
// tile, each taking every KS-th (8-channel group, tap) sub-step; partial accumulators are summed through LDS.
template <int WCO, int WPX, int TCO, int TPX, int KS = 1>
__global__ __launch_bounds__(512, (TCO * TPX <= 3) ? 4 : 2) void conv_igemm_kernel(const ConvDesc d) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  static_assert(WCO * WPX * KS == 4, "4 MFMA waves per workgroup");
  constexpr int BCO_T = WCO * TCO;
  // small tiles: pipeline steps of TS (8-channel group, tap) sub-steps so that a step carries >= 8-12 MFMAs
  constexpr int TS = (TCO * TPX == 1) ? 3 : ((TCO * TPX == 2) ? 2 : 1);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool loader = wave >= 4;
  const ConvPtrs P = d.g[blockIdx.y];
  const PatchGeom& pg = d.pg;

  // XCD-aware tile order: the co-blocks of one pixel tile and the vertically adjacent tiles (which share most of their
  // halo rows) meet in the same L2
  int bid = xcd_block_id();
  const int cb = bid % d.ncb;
  int pt = bid / d.ncb;
  const int tx_i = pt % d.tiles_x;
  pt /= d.tiles_x;
  const int ty_i = pt % d.tiles_y;
  const int tn_i = pt / d.tiles_y;
  const int ox0 = tx_i << d.lgTW, oy0 = ty_i << d.lgTH, n0 = tn_i << d.lgTI;
  const int S_in = pg.S == 2 ? 2 : 1;
  const int iyb = oy0 * S_in + d.iy0, ixb = ox0 * S_in + d.ix0;
  const int bufsz = d.ckm * 8 * pg.CS;
  const int nchunks = (d.nchunks8 + d.ckm - 1) / d.ckm;

  if (loader) {
    const int lw = __builtin_amdgcn_readfirstlane(wave) - 4;
    PlaneMap pm;

    if (pg.dma) {
      // activation-free operand with a linear patch layout: LDS-DMA (global_load_lds_dword).  No VGPR holds the data,
      // so a loader wave keeps every element of its channels in flight at once instead of 12-16 loads per lane; the
      // wave drains vmcnt before the barrier that publishes the buffer (barriers do not wait for DMAs)
      plane_map_init(pm, pg, n0, iyb, ixb, lane);
      stage_planes_dma(P.x, pm, pg, 0, min(d.ckm, d.nchunks8) * 8, smem, lw, lane);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      for (int chunk = 0; chunk < nchunks; ++chunk) {
        if (chunk + 1 < nchunks) {
          const int c8 = (chunk + 1) * d.ckm;
          stage_planes_dma(P.x, pm, pg, c8 * 8, min(d.ckm, d.nchunks8 - c8) * 8, smem + ((chunk + 1) & 1) * bufsz, lw, lane);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
      }
      return;
    }
    if (pg.vec4) {
      plane_map_init_v4(pm, pg, n0, iyb, ixb, lane);
      stage_planes_v4<8>(P.x, pm, pg, 0, min(d.ckm, d.nchunks8) * 8, smem, lw);
      __syncthreads();
      for (int chunk = 0; chunk < nchunks; ++chunk) {
        if (chunk + 1 < nchunks) {
          const int c8 = (chunk + 1) * d.ckm;
          stage_planes_v4<8>(P.x, pm, pg, c8 * 8, min(d.ckm, d.nchunks8 - c8) * 8, smem + ((chunk + 1) & 1) * bufsz,
                             lw);
        }
        __syncthreads();
      }
      return;
    }
    plane_map_init(pm, pg, n0, iyb, ixb, lane);
    stage_planes<12>(P.x, pm, pg, 0, min(d.ckm, d.nchunks8) * 8, smem, lw);
    __syncthreads();
    for (int chunk = 0; chunk < nchunks; ++chunk) {
      if (chunk + 1 < nchunks) {
        const int c8 = (chunk + 1) * d.ckm;
        stage_planes<12>(P.x, pm, pg, c8 * 8, min(d.ckm, d.nchunks8 - c8) * 8, smem + ((chunk + 1) & 1) * bufsz, lw);
      }
      __syncthreads();
    }
    return;
  }

  // ------------------------------------------------------------------ MFMA waves
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);   // wave-uniform: step bookkeeping stays on the scalar unit
  const int wk = wave_u % KS, wsp = wave_u / KS;   // K-split index, spatial wave index
  const int wco = wsp / WPX, wpx = wsp % WPX;
  const int h = lane >> 5, l31 = lane & 31;
  const int TWm = (1 << d.lgTW) - 1, THm = (1 << d.lgTH) - 1;
  const int rowmul = S_in * pg.PWrow;
  int boff[TPX];
#pragma unroll
  for (int tp = 0; tp < TPX; ++tp) {
    const int p = (wpx * TPX + tp) * 32 + l31;
    const int tx = p & TWm, ty = (p >> d.lgTW) & THm, ti = p >> (d.lgTW + d.lgTH);
    boff[tp] = h * pg.CS + ti * pg.PP + ty * rowmul + tx;
  }
  f32x16 acc[TCO][TPX];
#pragma unroll
  for (int a = 0; a < TCO; ++a)
#pragma unroll
    for (int b = 0; b < TPX; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;

  const char* wbase = reinterpret_cast<const char*>(P.wp);   // wave-uniform: weight loads are saddr + 32-bit voffset
  const int cot0 = cb * BCO_T + wco * TCO;
  unsigned wl[TCO];  // per-lane byte offset of the fragment of co tile a inside one (chunk8, tap) step
#pragma unroll
  for (int a = 0; a < TCO; ++a) wl[a] = (unsigned)(min(cot0 + a, d.ncot - 1) * 64 + lane) * 16u;
  const long long qstride = (long long)d.ncot * 64 * 16;   // bytes between consecutive (chunk8, tap) steps
  const int Qtot = d.nchunks8 * d.ntaps;
  {
    // LDS offset of sub-step q of a chunk (8-channel group q / ntaps, tap q % ntaps) lives in lane q of one VGPR:
    // v_readlane replaces the scalar (group, tap) bookkeeping; the host guarantees ckm * ntaps <= 64
    int step_lane;
    {
      const int sq = lane / d.ntaps, tq = lane - sq * d.ntaps;
      step_lane = sq * 8 * pg.CS + d.tapoff[tq];
    }
    // Pipeline over steps of TS (8-channel group, tap) sub-steps (small tiles take TS > 1 so that a step carries
    // >= 8-12 MFMAs).  A fragments (packed weights) come from L2, whose latency exceeds one step of a small tile:
    // they are prefetched TWO steps ahead into two register sets used alternately (the step loop is unrolled by two,
    // chunks are padded to an even number of steps with zeroed B fragments).  B fragments come from LDS one step ahead.
    auto chunk_nq = [&](int c) { return min(d.ckm, d.nchunks8 - c * d.ckm) * d.ntaps; };
    // scalar pointer to the packed weights of sub-step u of step `st` of chunk `c` (st may run past the chunk:
    // first steps of the next chunk; past the end: clamped, never used)
    // sub-steps of a chunk taken by this wave: q = wk, wk + KS, ...; padded to an even number of steps
    auto steps2 = [&](int nq_c) { return ((((nq_c - wk + KS - 1) / KS) + TS - 1) / TS + 1) & ~1; };
    auto wptr = [&](int c, int st, int u) -> const char* {
      int nq_c = chunk_nq(c);
      const int ns2 = steps2(nq_c);
      if (st >= ns2) {
        st -= ns2;
        c += 1;
        nq_c = (c < nchunks) ? chunk_nq(c) : 1;
      }
      const int qw = min(c * d.ckm * d.ntaps + min((st * TS + u) * KS + wk, nq_c - 1), Qtot - 1);
      return wbase + qw * qstride;
    };
    f32x4 aq0[TS][TCO], aq1[TS][TCO];
#pragma unroll
    for (int u = 0; u < TS; ++u)
#pragma unroll
      for (int a = 0; a < TCO; ++a) {
        aq0[u][a] = *reinterpret_cast<const f32x4*>(wptr(0, 0, u) + wl[a]);
        aq1[u][a] = *reinterpret_cast<const f32x4*>(wptr(0, 1, u) + wl[a]);
      }

    __syncthreads();  // patch of chunk 0 staged
    for (int chunk = 0; chunk < nchunks; ++chunk) {
      const float* cur = smem + (chunk & 1) * bufsz;
      const int nq = chunk_nq(chunk);
      const int nsteps2 = steps2(nq);
      float bv_n[TS][4][TPX];
      float ok_n[TS];   // 1 / 0 (wave-uniform): sub-steps past the chunk contribute zero; applied when bv_n is consumed
      // B fragments of sub-step u of step st of this chunk into bv_n
      auto bload = [&](int st, int u) {
        const int qq = (st * TS + u) * KS + wk;
        const int qc = min(qq, nq - 1);
        ok_n[u] = (qq < nq) ? 1.0f : 0.0f;
        const float* bp = cur + __builtin_amdgcn_readlane(step_lane, qc);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int tp = 0; tp < TPX; ++tp) bv_n[u][j][tp] = bp[boff[tp] + 2 * j * pg.CS];
      };
      // One step with register set `aq`.  Source order IS the issue order (sched_barrier pins each group): the four
      // k-pairs of a weight fragment issue back to back, then -- while the matrix pipe works them off -- the LDS
      // reads of the next step's B fragments and the refill of this fragment with the weights two steps ahead.
      auto half_step = [&](f32x4 (&aq)[TS][TCO], int st) {
        float bv[TS][4][TPX];
#pragma unroll
        for (int u = 0; u < TS; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int tp = 0; tp < TPX; ++tp) bv[u][j][tp] = bv_n[u][j][tp] * ok_n[u];
        const int stn = min(st + 1, nsteps2 - 1);
#pragma unroll
        for (int u = 0; u < TS; ++u) {
          const char* sp = wptr(chunk, st + 2, u);
#pragma unroll
          for (int a = 0; a < TCO; ++a) {
#pragma unroll
            for (int tp = 0; tp < TPX; ++tp)
#pragma unroll
              for (int j = 0; j < 4; ++j)
                acc[a][tp] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[u][a][j], bv[u][j][tp], acc[a][tp], 0, 0, 0);
            if (a == 0) bload(stn, u);
            aq[u][a] = *reinterpret_cast<const f32x4*>(sp + wl[a]);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      };
#pragma unroll
      for (int u = 0; u < TS; ++u) bload(0, u);
      for (int st = 0; st < nsteps2; st += 2) {
        half_step(aq0, st);
        half_step(aq1, st + 1);
      }
      __syncthreads();
    }
  }

  if constexpr (KS > 1) {
    // split-K reduction: the staging buffers are free after the last chunk barrier (the loaders have left: ended
    // waves do not take part in s_barrier).  Waves wk > 0 park their accumulators in LDS, wave wk == 0 adds them.
    static_assert(TCO == 1 && TPX == 1, "split-K configurations hold one tile per wave");
    float* red = smem + (wsp * (KS - 1)) * 1024;
    if (wk > 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) red[(wk - 1) * 1024 + r * 64 + lane] = acc[0][0][r];
    }
    __syncthreads();
    if (wk > 0) return;
#pragma unroll
    for (int k = 0; k < KS - 1; ++k)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][0][r] += red[k * 1024 + r * 64 + lane];
  }
  // ---- epilogue: D[row = co][col = pixel]; lane holds column l31, rows (r&3)+8*(r>>2)+4*h
  {
    int pn[TPX], poy[TPX], pox[TPX];
    bool pv[TPX];
#pragma unroll
    for (int tp = 0; tp < TPX; ++tp) {
      const int p = (wpx * TPX + tp) * 32 + l31;
      const int tx = p & TWm, ty = (p >> d.lgTW) & THm, ti = p >> (d.lgTW + d.lgTH);
      const int oyv = oy0 + ty, oxv = ox0 + tx;
      pn[tp] = n0 + ti;
      pv[tp] = (pn[tp] < d.pg.N) && (oyv < d.OHv) && (oxv < d.OWv);
      poy[tp] = oyv * d.out_sy + d.out_oy;
      pox[tp] = oxv * d.out_sx + d.out_ox;
    }
    epilogue_dispatch<TCO, TPX>(d, P, acc, cot0, h, pn, poy, pox, pv);
  }
}

// ------------------------------------------------------------------------------------------------
// weight packing: wp[((chunk*ntaps + t)*ncot + cot)*64 + lane][j] = W[co = cot*32 + (lane&31)]
//                                                                    [ci = chunk*8 + 2*j + (lane>>5)][tap t]
struct PackDesc {
  const float* w;
  float* wp;
  int Co, Ci, KHW, src_out_major, ntaps, ncot, nchunks, nonneg;
  float bound, pedestal;
  int src_ld, src_off;          // sub-matrix of a wider weight: row length / first entry of the inner matrix index
  int dst_ncot, dst_cot_off;    // concatenation along GEMM-M: tiles per step of the destination, first tile of this job
  int wino;                     // 0: spatial taps; 1 / 2: Winograd F(2x2,3x3) weights U = G g G^T of the 3x3 kernel (2: of
                                // the 180-degree rotated kernel = input-gradient orientation): 16 "taps" = transform points
  int cg, ngroups;              // an item = (32-co tile, cg consecutive 8-ci chunks); ngroups = ceil(nchunks / cg)
  int vec;                      // every source row of every item starts on a 16-byte boundary
  short tapidx[ICM_MAX_TAPS];
};

// One item = one workgroup = (32-co tile, cg 8-ci chunks): the source block is read row by row into LDS (row stride
// padded to an odd number of words), then written out in fragment order.  The canonical layouts differ only in which index
// is the contiguous row: W[co][ci][khw] (src_out_major: 32 rows of 8*cg*KHW) or W[ci][co][khw] (8*cg rows of 32*KHW).
//   * every row goes to 256 / rows threads: no division in the loop, 16-byte loads where the job's rows are aligned
//     (dwords otherwise and for a row's last 1-3 floats), four (vector) or eight (dword) independent loads in flight;
//   * thread p owns the weight pair (co = (p >> 2) & 31, ci = 2 (p & 3) + (p >> 7)) of each chunk: float p of the 1 KB
//     fragment block of every tap, so a tap's block leaves as 256 consecutive dwords -- four per 16-byte fragment entry --
//     and the Winograd transform of a pair is formed once, by its thread, from nine LDS reads;
//   * nothing loops over items: a launch's items go to the hardware dispatcher one workgroup each, LDS sized by the
//     launch's largest source block, so small and large jobs of one launch fill the CUs together.
__host__ __device__ inline int pack_lds_floats(int cg, int KHW) { return 256 * cg * KHW + 32; }

__device__ __forceinline__ float pack_nonneg(float x, float bound, float pedestal) {
  x = fmaxf(x, bound);
  x = x * x - pedestal;
  return x;
}

// U[a][b] = sum_pq G[a][p] g[p][q] G[b][q],  G = [[1,0,0],[1/2,1/2,1/2],[1/2,-1/2,1/2],[0,0,1]]   (u[4 a + b]) of one
// 3x3 kernel g (wino == 2: of the kernel rotated by 180 degrees).  Every product and sum is rounded on its own: with the
// row and the column half in one expression tree the compiler would fuse 0.5 * x of the row half into the column sums.
__device__ __forceinline__ void pack_wino_points(const float* g, int wino, float (&u)[16]) {
#pragma clang fp contract(off)
  float row[3][4];   // (g G^T)[p][b]
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    const float g0 = g[wino == 2 ? (2 - p) * 3 + 2 : p * 3 + 0];
    const float g1 = g[wino == 2 ? (2 - p) * 3 + 1 : p * 3 + 1];
    const float g2 = g[wino == 2 ? (2 - p) * 3 + 0 : p * 3 + 2];
    row[p][0] = g0;
    row[p][1] = 0.5f * ((g0 + g2) + g1);
    row[p][2] = 0.5f * ((g0 + g2) - g1);
    row[p][3] = g2;
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    u[0 * 4 + b] = row[0][b];
    u[1 * 4 + b] = 0.5f * ((row[0][b] + row[2][b]) + row[1][b]);
    u[2 * 4 + b] = 0.5f * ((row[0][b] + row[2][b]) - row[1][b]);
    u[3 * 4 + b] = row[2][b];
  }
}

__device__ __forceinline__ void pack_item(const PackDesc& d, int item, float* lds) {
  const int KHW = d.KHW, tid = threadIdx.x;
  const int cot = item % d.ncot, grp = item / d.ncot;
  const int co0 = cot * 32, chunk0 = grp * d.cg, ci0 = chunk0 * 8;
  const int nch = min(d.cg, d.nchunks - chunk0);            // chunks of this item
  const int som = d.src_out_major;
  const int rows = som ? 32 : 8 * d.cg;                     // 8 or 32
  const int lgt = rows == 32 ? 3 : 5, tpr = 1 << lgt;       // threads per row
  const int rlen = som ? 8 * d.cg * KHW : 32 * KHW, rstride = rlen | 1;
  {
    const int r = tid >> lgt, c0 = tid & (tpr - 1);
    const int outer = (som ? co0 : ci0) + r, inner0 = som ? ci0 : co0;
    const bool rok = outer < (som ? d.Co : d.Ci);
    const int len = rok ? min(som ? 8 * nch : 32, (som ? d.Ci : d.Co) - inner0) * KHW : 0;   // floats of the row that exist
    const float* src = d.w + ((long long)outer * d.src_ld + d.src_off + inner0) * KHW;
    float* dst = lds + r * rstride;
    const int n4 = d.vec ? len >> 2 : 0;
    for (int b = c0; b < n4; b += 4 * tpr) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (b + u * tpr < n4) v[u] = *reinterpret_cast<const f32x4*>(src + 4 * (b + u * tpr));
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (b + u * tpr < n4) {
#pragma unroll
          for (int i = 0; i < 4; ++i) dst[4 * (b + u * tpr) + i] = d.nonneg ? pack_nonneg(v[u][i], d.bound, d.pedestal) : v[u][i];
        }
    }
    for (int b = 4 * n4 + c0; b < len; b += 8 * tpr) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (b + u * tpr < len) v[u] = src[b + u * tpr];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (b + u * tpr < len) dst[b + u * tpr] = d.nonneg ? pack_nonneg(v[u], d.bound, d.pedestal) : v[u];
    }
  }
  __syncthreads();
  const int col = (tid >> 2) & 31, cil = 2 * (tid & 3) + (tid >> 7);
  const long long tstride = (long long)d.dst_ncot * 256;   // floats between the blocks of consecutive taps
  for (int cc = 0; cc < nch; ++cc) {
    const int cl = cc * 8 + cil;
    const float* gsrc = som ? lds + col * rstride + cl * KHW : lds + cl * rstride + col * KHW;
    const bool valid = (co0 + col < d.Co) && (ci0 + cl < d.Ci);   // padded rows / channels are exact zeros (also under nonneg)
    float* out = d.wp + ((long long)(chunk0 + cc) * d.ntaps * d.dst_ncot + d.dst_cot_off + cot) * 256 + tid;
    if (d.wino) {
      float u[16];
      pack_wino_points(gsrc, d.wino, u);
#pragma unroll
      for (int t = 0; t < 16; ++t) out[t * tstride] = valid ? u[t] : 0.0f;
    } else {
      for (int t = 0; t < d.ntaps; ++t) out[t * tstride] = valid ? gsrc[d.tapidx[t]] : 0.0f;
    }
  }
}

__global__ __launch_bounds__(256) void pack_weights_kernel(const PackDesc d) {
  extern __shared__ float pack_lds[];
  pack_item(d, blockIdx.x, pack_lds);
}

#define ICM_PACK_NB 24
struct PackMulti {
  PackDesc g[ICM_PACK_NB];
  int first[ICM_PACK_NB];   // first item of job i in the launch's flat item list (INT_MAX behind the last job)
};
static_assert(sizeof(PackMulti) <= 4096, "kernel arguments are passed by value");
__global__ __launch_bounds__(256) void pack_weights_multi_kernel(const PackMulti m) {
  extern __shared__ float pack_lds[];
  const int item = blockIdx.x;
  int job = 0;
#pragma unroll
  for (int i = 1; i < ICM_PACK_NB; ++i) job += item >= m.first[i];
  pack_item(m.g[job], item - m.first[job], pack_lds);
}

// ---------------------------------------------------------------------------------- host planning
struct Tap {
  int kidx;    // kh*KW + kw in the canonical weight
  int dy, dx;  // patch-relative offsets
};
struct ConvClass {
  int cy, cx;      // output parity (scatter) -- 0,0 for gather
  int iy0, ix0;    // input coordinate of patch row/col 0 for virtual output 0
  int ey, ex;      // patch extents contributed by taps (max dy + 1)
  std::vector<Tap> taps;
};

// Taps of one axis for output parity c of a scatter conv: k with (c + pad - k) % s == 0, input offset (c+pad-k)/s
static void axis_taps(int K, int s, int pad, int c, std::vector<int>& ks, std::vector<int>& dis) {
  for (int k = 0; k < K; ++k) {
    const int v = c + pad - k;
    if (((v % s) + s) % s != 0) continue;
    ks.push_back(k);
    dis.push_back(v >= 0 ? v / s : -((-v) / s));
  }
}

static std::vector<ConvClass> build_classes(int KH, int KW, int stride, int pad, int transposed) {
  std::vector<ConvClass> out;
  if (!transposed) {
    ConvClass c;
    c.cy = c.cx = 0;
    c.iy0 = c.ix0 = -pad;
    c.ey = KH;
    c.ex = KW;
    for (int kh = 0; kh < KH; ++kh)
      for (int kw = 0; kw < KW; ++kw) c.taps.push_back({kh * KW + kw, kh, kw});
    out.push_back(c);
    return out;
  }
  for (int cy = 0; cy < stride; ++cy)
    for (int cx = 0; cx < stride; ++cx) {
      std::vector<int> khs, dys, kws, dxs;
      axis_taps(KH, stride, pad, cy, khs, dys);
      axis_taps(KW, stride, pad, cx, kws, dxs);
      ConvClass c;
      c.cy = cy;
      c.cx = cx;
      int miny = 0, minx = 0, maxy = 0, maxx = 0;
      for (size_t i = 0; i < dys.size(); ++i) {
        miny = i ? std::min(miny, dys[i]) : dys[i];
        maxy = i ? std::max(maxy, dys[i]) : dys[i];
      }
      for (size_t i = 0; i < dxs.size(); ++i) {
        minx = i ? std::min(minx, dxs[i]) : dxs[i];
        maxx = i ? std::max(maxx, dxs[i]) : dxs[i];
      }
      c.iy0 = miny;
      c.ix0 = minx;
      c.ey = maxy - miny + 1;
      c.ex = maxx - minx + 1;
      for (size_t a = 0; a < khs.size(); ++a)
        for (size_t b = 0; b < kws.size(); ++b)
          c.taps.push_back({khs[a] * KW + kws[b], dys[a] - miny, dxs[b] - minx});
      out.push_back(c);
    }
  return out;
}

// One row per instantiation; the index is the id of icm_debug_force_conv_cfg.  Cost model inputs: eff = efficiency measured
// on MI355X (tools/tune_conv.py; profiles/r01_tune_conv_v7.txt), occ = 2 where the kernel fits 128 VGPRs (launch bounds)
struct KernelCfg {
  int wco, wpx, tco, tpx;
  void (*fn)(const ConvDesc);
  int ks;   // intra-workgroup K split
  double eff;
  int occ;
};
static const KernelCfg kCfgs[] = {
    {1, 4, 3, 2, conv_igemm_kernel<1, 4, 3, 2>, 1, 0.75, 1},     // 96 co x 256 px
    {1, 4, 6, 1, conv_igemm_kernel<1, 4, 6, 1>, 1, 1.00, 1},     // 192 x 128
    {1, 4, 2, 2, conv_igemm_kernel<1, 4, 2, 2>, 1, 0.80, 1},     // 64 x 256
    {1, 4, 1, 2, conv_igemm_kernel<1, 4, 1, 2>, 1, 0.60, 2},     // 32 x 256
    {1, 4, 3, 1, conv_igemm_kernel<1, 4, 3, 1>, 1, 1.10, 2},     // 96 x 128
    {1, 4, 5, 1, conv_igemm_kernel<1, 4, 5, 1>, 1, 0.65, 1},     // 160 x 128
    {2, 2, 2, 1, conv_igemm_kernel<2, 2, 2, 1>, 1, 0.80, 2},     // 128 x 64
    {2, 2, 1, 1, conv_igemm_kernel<2, 2, 1, 1>, 1, 0.80, 2},     // 64 x 64
    {4, 1, 1, 1, conv_igemm_kernel<4, 1, 1, 1>, 1, 0.75, 2},     // 128 x 32
    {1, 4, 1, 1, conv_igemm_kernel<1, 4, 1, 1>, 1, 0.70, 2},     // 32 x 128
    {2, 1, 1, 1, conv_igemm_kernel<2, 1, 1, 1, 2>, 2, 0.70, 2},  // 64 x 32, K split in 2
    {1, 2, 1, 1, conv_igemm_kernel<1, 2, 1, 1, 2>, 2, 0.70, 2},  // 32 x 64, K split in 2
    {1, 1, 1, 1, conv_igemm_kernel<1, 1, 1, 1, 4>, 4, 0.65, 2},  // 32 x 32, K split in 4
};
constexpr int kNumCfgs = (int)(sizeof(kCfgs) / sizeof(kCfgs[0]));
static_assert(kNumCfgs <= ICM_CONV_CFG_KS8_64X64, "the K-split ids lie above the table rows");

static int g_force_cfg = ICM_CONV_CFG_AUTO;
static bool cfg_forced() { return g_force_cfg != ICM_CONV_CFG_AUTO; }
static bool ks8_forced() { return g_force_cfg == ICM_CONV_CFG_KS8_64X64 || g_force_cfg == ICM_CONV_CFG_KS8_32X128; }
static bool row_forced() { return cfg_forced() && g_force_cfg < ICM_CONV_CFG_KS8_64X64; }
static int g_force_1x1 = env_int("ICM_CONV_1X1", -1);   // -1 auto, 0 never, 1 whenever eligible

static Geometry make_geometry(int bpx, int OHv, int OWv, int N, int S, int ey, int ex, int nchunks8, int ntaps,
                              int tiles_per_wave) {
  Geometry g;
  const int lgB = ceil_log2(bpx);
  g.lgTW = std::min(std::min(5, lgB), ceil_log2(OWv));
  g.lgTH = std::min(lgB - g.lgTW, ceil_log2(OHv));
  g.lgTI = lgB - g.lgTW - g.lgTH;
  const int TW = 1 << g.lgTW, TH = 1 << g.lgTH, TI = 1 << g.lgTI;
  g.PW = (TW - 1) * S + ex;
  g.PH = (TH - 1) * S + ey;
  g.PWh = (g.PW + 1) / 2;
  g.PWrow = (S == 2) ? 2 * g.PWh : g.PW;
  g.PP = g.PH * g.PWrow;
  g.CS = TI * g.PP;
  g.tiles_x = cdiv(OWv, TW);
  g.tiles_y = cdiv(OHv, TH);
  g.tiles_n = cdiv(N, TI);
  // channels per barrier: >= ~256 MFMAs per MFMA wave between barriers (16k cycles) so that the loaders' L2/HBM
  // round trips and the barrier itself stay hidden, within 64 KB of LDS for the two buffers
  int ckm = cdiv(256, ntaps * 4 * tiles_per_wave);
  ckm = std::max(1, std::min(ckm, nchunks8));
  ckm = std::max(1, std::min(ckm, 64 / std::max(1, ntaps)));   // step table = one VGPR (64 lanes)
  while (ckm > 1 && (size_t)2 * ckm * 8 * g.CS * sizeof(float) > 64 * 1024) --ckm;
  g.ckm = ckm;
  g.lds_bytes = (size_t)2 * ckm * 8 * g.CS * sizeof(float);
  return g;
}
static bool fits_plane_map(const Geometry& g) { return (1 << g.lgTI) * g.PH * g.PW <= ICM_MAXJ * 64; }
static bool linear_patch(const Geometry& g) { return g.PWrow == g.PW && g.PP == g.PH * g.PW; }
static long long tile_count(const Geometry& g) { return (long long)g.tiles_x * g.tiles_y * g.tiles_n; }

struct ClassShape { int OHv, OWv, ncot, nchunks8, ntaps; };   // virtual output grid (a scatter class writes every out_s-th row / column)
static ClassShape class_shape(const icm_conv_args& a, const ConvClass& cls, int out_s) {
  return {a.transposed ? cdiv(a.OH - cls.cy, out_s) : a.OH, a.transposed ? cdiv(a.OW - cls.cx, out_s) : a.OW,
          cdiv(a.Cout, 32), cdiv(a.Cin, 8), (int)cls.taps.size()};
}

// Tile configuration of the staged kernel: time ~ rounds x (co-resident workgroups share the MFMA pipes: occ x MFMAs per
// wave / efficiency + one fixed prologue/epilogue overhead per round), rounds = ceil(workgroups / (256 CUs x occ)).
static int search_staged(const icm_conv_args& a, int ngroups, const ConvClass& cls, const ClassShape& s, int S_in,
                         Geometry& bg) {
  static const double kCoResBoost = env_double("ICM_CONV_BOOST", 1.25);
  int best = -1, best1 = -1;
  double best_cost = 1e300, best1_cost = 1e300;
  Geometry bg1{};
  for (int i = 0; i < kNumCfgs; ++i) {
    if (row_forced() && i != g_force_cfg) continue;
    const KernelCfg& c = kCfgs[i];
    const int bpx = c.wpx * c.tpx * 32, bco_t = c.wco * c.tco;
    Geometry g = make_geometry(bpx, s.OHv, s.OWv, a.N, S_in, cls.ey, cls.ex, s.nchunks8, s.ntaps, c.tco * c.tpx);
    if (c.ks > 1) g.lds_bytes = std::max<size_t>(g.lds_bytes, (size_t)(c.ks - 1) * c.wco * c.wpx * 4096);
    if (g.lds_bytes > 160 * 1024 || !fits_plane_map(g)) continue;
    const long long blocks = cdiv(s.ncot, bco_t) * tile_count(g) * ngroups;
    const int occ_max = (g.lds_bytes * 2 <= 160 * 1024) ? c.occ : 1;
    const int occ = (int)std::min<long long>(occ_max, (blocks + 255) / 256);   // workgroups actually co-resident
    const double rounds = (double)((blocks + 256 * occ - 1) / (256 * occ));
    const double mfma = (double)c.tco * c.tpx * s.nchunks8 * s.ntaps * 4 / c.ks + (c.ks > 1 ? 24.0 : 0.0);   // per MFMA wave
    // two co-resident workgroups interleave their MFMA streams: the issue gaps of one wave per SIMD are filled
    // (the interleaving gain fades for long K loops, whose steady state already keeps the matrix pipe busy)
    const double boost = occ > 1 ? 1.0 + (kCoResBoost - 1.0) * std::min(1.0, 1500.0 / mfma) : 1.0;
    const double cost = rounds * (occ * mfma / (c.eff * boost) + 200.0);
    // a configuration whose co-tile covers all output channels stages every halo patch exactly once
    if (s.ntaps >= 9 && (long long)s.OHv * s.OWv * a.N >= 16384 && cdiv(s.ncot, bco_t) == 1 && cost < best1_cost) {
      best1_cost = cost;
      best1 = i;
      bg1 = g;
    }
    if (cost < best_cost) {
      best_cost = cost;
      best = i;
      bg = g;
    }
  }
  // halo convolutions with many pixels: within 20 % of the cheapest estimate, take the single-pass-over-activations
  // tiling (every extra co-block re-stages the whole halo patch from L2 / HBM: 1.85x FETCH_SIZE measured on g_a.2
  // for 3 % of MFMA time)
  if (best1 >= 0 && best1_cost <= 1.2 * best_cost) {
    best = best1;
    bg = bg1;
  }
  return best;
}

// Latency-bound launches: the 8-wave K-split kernel (conv_ks8.hip).  Needs stride-1 sampling, no operand activation,
// the GDN / AXPY2 epilogues excluded (they belong to pointwise launches), and the step table in one VGPR
// (ckm * ntaps <= 64, as here).  It runs one workgroup per CU, so it is taken only when its grid is ONE nearly full
// round of the chip (160..256 workgroups): there it cuts the critical path of the serial slice-chain layers by ~15 %
// (224 -> 176 @16x16: 60 -> 51 us, 480 -> 224: 116 -> 100 us); applied to every small launch it lost 1.3 % on the
// step (narrow outputs 64 -> 32: 17 -> 29 us, half-empty grids, second-round tails; same-box A/B).
// Returns its co tiles per block; 0: the launch keeps the staged kernel.
static int plan_ks8(const icm_conv_args& a, int ngroups, const ConvClass& cls, const ClassShape& s, int S_in, Geometry& g) {
  static const int ks8_on = env_int("ICM_CONV_KS8", 1);
  static const long long ks8_max = env_ll("ICM_CONV_KS8_MAXWG", 256);
  static const long long ks8_min = env_ll("ICM_CONV_KS8_MINWG", 160);
  if (!(ks8_forced() || (ks8_on && !cfg_forced())) || S_in != 1 || s.ntaps <= 1 || a.pro_act != ICM_ACT_NONE ||
      !EpiKs8::has(a.epi) || a.x_seg_len != 0)
    return 0;
  const int tco = g_force_cfg == ICM_CONV_CFG_KS8_32X128 ? 1 : (g_force_cfg == ICM_CONV_CFG_KS8_64X64 ? 2 : (s.ncot >= 2 ? 2 : 1));
  g = make_geometry(tco == 2 ? 64 : 128, s.OHv, s.OWv, a.N, S_in, cls.ey, cls.ex, s.nchunks8, s.ntaps, 4);
  // more K per barrier than the staged kernel needs: every wave should find >= 2 of its sub-steps in a chunk
  int ckm = std::max(1, std::min(s.nchunks8, 64 / s.ntaps));
  while (ckm > 1 && (size_t)2 * ckm * 8 * g.CS * sizeof(float) > 96 * 1024) --ckm;
  g.ckm = ckm;
  g.lds_bytes = std::max((size_t)2 * ckm * 8 * g.CS * sizeof(float), (size_t)8 * 4 * 16 * 64 * sizeof(float));
  const long long blocks = cdiv(s.ncot, tco) * tile_count(g) * ngroups;
  const bool fits = g.lds_bytes <= 160 * 1024 && fits_plane_map(g) && linear_patch(g);
  return (fits && (ks8_forced() || (blocks <= ks8_max && blocks >= ks8_min && tco == 2))) ? tco : 0;
}

// Everything one tap class's launch decides; no HIP call, no pointer read.  Precedence: the pointwise kernel unless a
// configuration is forced, the cost search, the K-split override (its own geometry).  p.nblk == 0: an empty class.
static int plan_class(const icm_conv_args& a, int ngroups, const ConvClass& cls, int S_in, int out_s, bool x_aligned16,
                      ConvPlan& p) {
  p = ConvPlan{};
  const ClassShape s = class_shape(a, cls, out_s);
  if (s.OHv <= 0 || s.OWv <= 0) return ICM_OK;
  if (s.ntaps > ICM_MAX_TAPS) return ICM_ERR_UNSUPPORTED;
  if (s.ntaps == 1 && S_in == 1 && out_s == 1 && cls.iy0 == 0 && cls.ix0 == 0 && a.x_seg_len == 0 && !cfg_forced()) {
    const int rc = plan_conv1x1(a, ngroups, g_force_1x1, p);
    if (rc >= 0) return rc;
  }
  p.row = search_staged(a, ngroups, cls, s, S_in, p.g);
  if (p.row < 0) return ICM_ERR_UNSUPPORTED;
  p.block = 512;
  Geometry kg;
  if (const int tco = plan_ks8(a, ngroups, cls, s, S_in, kg)) {
    p.family = kFamKs8;
    p.row = tco;
    p.g = kg;
    p.dma = 1;
  } else {
    const Geometry& g = p.g;
    const int plane4 = (1 << g.lgTI) * g.PH * (g.PW / 4);
    // 16-byte halo-free staging (the packed vec4 form moves several channels per instruction: keep segments simple)
    p.vec4 = S_in == 1 && cls.ex == 1 && cls.ey == 1 && cls.ix0 == 0 && (g.PW % 4) == 0 && ((1 << g.lgTW) % 4) == 0 &&
             (a.W % 4) == 0 && (a.x_bs % 4) == 0 && ((long long)a.H * a.W % 4) == 0 && plane4 <= 4 * 64 &&
             (g.CS % 4) == 0 && (g.PWrow % 4) == 0 && (g.PP % 4) == 0 && x_aligned16 && a.x_seg_len == 0;
    // LDS-DMA staging: no activation to apply, linear patch layout (stride-1 input sampling: no column-parity split),
    // not the 16-byte halo-free path (4x the bytes per instruction)
    static const int dma_on = env_int("ICM_CONV_DMA", 1);
    p.dma = dma_on && !p.vec4 && S_in == 1 && a.pro_act == ICM_ACT_NONE && linear_patch(g);
  }
  p.ncb = cdiv(s.ncot, p.family == kFamKs8 ? p.row : kCfgs[p.row].wco * kCfgs[p.row].tco);
  p.nblk = p.ncb * tile_count(p.g);
  if (p.nblk <= 0 || p.nblk > 0x7fffffffLL) return ICM_ERR_ARG;
  return ICM_OK;
}

static int launch_class(const icm_conv_args* arr, int ngroups, const ConvClass& cls, long long wp_off, int S_in,
                        int out_s, const ConvPlan& p, hipStream_t stream) {
  if (p.nblk == 0) return ICM_OK;
  const icm_conv_args& a = arr[0];
  ConvDesc d{};
  fill_conv_desc(d, arr, ngroups, wp_off);
  d.ncb = p.ncb;
  if (p.family == kFam1x1) return launch_conv1x1(d, a, p, ngroups, stream);
  const ClassShape s = class_shape(a, cls, out_s);
  const Geometry& bg = p.g;
  PatchGeom& pg = d.pg;
  pg.PW = bg.PW; pg.PH = bg.PH; pg.PWrow = bg.PWrow; pg.PWh = bg.PWh; pg.PP = bg.PP; pg.CS = bg.CS; pg.S = S_in;
  pg.TIPH = (1 << bg.lgTI) * bg.PH;
  pg.dPW = make_fastdiv((uint32_t)bg.PW);
  pg.dTIPH = make_fastdiv((uint32_t)pg.TIPH);
  pg.dPH = make_fastdiv((uint32_t)bg.PH);
  pg.H = a.H; pg.W = a.W; pg.N = a.N; pg.C = a.Cin; pg.act = a.pro_act; pg.bs = a.x_bs;
  pg.seg_len = a.x_seg_len; pg.seg_gap = a.x_seg_len ? a.x_seg_gap : 0;
  pg.dseg = make_fastdiv((uint32_t)std::max(1, a.x_seg_len));
  pg.vec4 = p.vec4; pg.dma = p.dma; pg.pipe = 0;
  set_v4_pack(pg);
  d.ps2 = a.pixel_shuffle == 2;
  d.OHf = d.ps2 ? a.OH * 2 : a.OH;
  d.OWf = d.ps2 ? a.OW * 2 : a.OW;
  d.OHv = s.OHv; d.OWv = s.OWv;
  d.out_sy = d.out_sx = out_s;
  d.out_oy = cls.cy; d.out_ox = cls.cx;
  d.iy0 = cls.iy0; d.ix0 = cls.ix0;
  d.ntaps = s.ntaps;
  d.lgTW = bg.lgTW; d.lgTH = bg.lgTH; d.lgTI = bg.lgTI;
  d.tiles_x = bg.tiles_x; d.tiles_y = bg.tiles_y; d.tiles_n = bg.tiles_n;
  d.nchunks8 = s.nchunks8; d.ckm = bg.ckm;
  for (int t = 0; t < s.ntaps; ++t) {
    const Tap& tp = cls.taps[t];
    const int col = (S_in == 2) ? ((tp.dx & 1) * bg.PWh + (tp.dx >> 1)) : tp.dx;
    d.tapoff[t] = tp.dy * bg.PWrow + col;
  }
  if (p.family == kFamKs8) return launch_conv_ks8(d, p.row, p.nblk, ngroups, bg.lds_bytes, stream);
  const KernelCfg& c = kCfgs[p.row];
  if (bg.lds_bytes > 64 * 1024 && !ensure_max_lds(reinterpret_cast<const void*>(c.fn))) return ICM_ERR_LAUNCH;
  hipLaunchKernelGGL(c.fn, dim3((unsigned)p.nblk, ngroups, 1), dim3(p.block), bg.lds_bytes, stream, d);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

static int validate(const icm_conv_args& a) {
  if (!a.x || !a.wp || !a.y) return ICM_ERR_ARG;
  if (a.N <= 0 || a.Cin <= 0 || a.Cout <= 0 || a.H <= 0 || a.W <= 0 || a.OH <= 0 || a.OW <= 0) return ICM_ERR_ARG;
  if (a.KH <= 0 || a.KW <= 0 || a.KH * a.KW > ICM_MAX_TAPS) return ICM_ERR_UNSUPPORTED;
  if (a.stride != 1 && a.stride != 2) return ICM_ERR_UNSUPPORTED;
  if (!a.transposed) {
    if (a.OH != (a.H + 2 * a.pad - a.KH) / a.stride + 1 || a.OW != (a.W + 2 * a.pad - a.KW) / a.stride + 1)
      return ICM_ERR_ARG;
  }
  if ((epi_reads_res(a.epi) && !a.res) || (epi_reads_aux(a.epi) && !a.aux) || (epi_reads_aux2(a.epi) && !a.aux2))
    return ICM_ERR_ARG;
  if (((long long)a.N * a.x_bs + 8LL * a.H * a.W) * 4 >= (1LL << 31)) return ICM_ERR_UNSUPPORTED;   // PlaneMap byte offsets are int32
  if (a.pixel_shuffle != 0 && a.pixel_shuffle != 2) return ICM_ERR_UNSUPPORTED;
  if (a.pixel_shuffle == 2 && (a.Cout % 4 != 0 || a.transposed)) return ICM_ERR_ARG;
  if (a.x_seg_len < 0 || (a.x_seg_len > 0 && (a.x_seg_gap < 0 || a.x_seg_len >= 65536))) return ICM_ERR_ARG;
  return ICM_OK;
}

static int check_group(const icm_conv_args* arr, int ngroups) {
  if (!arr || ngroups < 1 || ngroups > ICM_MAX_GROUPS) return ICM_ERR_ARG;
  for (int i = 0; i < ngroups; ++i) {
    int rc = validate(arr[i]);
    if (rc) return rc;
  }
  const icm_conv_args& a = arr[0];
  // one launch, one geometry: every member must agree with arr[0] in everything but its pointers (the kernel takes
  // shapes, strides, epilogue kind and flags from arr[0]; a mismatching member would read / write out of bounds)
  for (int i = 1; i < ngroups; ++i) {
    const icm_conv_args& b = arr[i];
    if (b.N != a.N || b.Cin != a.Cin || b.H != a.H || b.W != a.W || b.Cout != a.Cout || b.OH != a.OH || b.OW != a.OW ||
        b.KH != a.KH || b.KW != a.KW || b.stride != a.stride || b.pad != a.pad || b.transposed != a.transposed ||
        b.pro_act != a.pro_act || b.epi != a.epi || b.accum != a.accum || b.pixel_shuffle != a.pixel_shuffle ||
        b.x_bs != a.x_bs || b.y_bs != a.y_bs || b.x_seg_len != a.x_seg_len || b.x_seg_gap != a.x_seg_gap || b.algo != a.algo ||
        (b.res && b.res_bs != a.res_bs) || (b.aux && b.aux_bs != a.aux_bs) || (b.aux2 && b.aux2_bs != a.aux2_bs) ||
        (b.y2 && b.y2_bs != a.y2_bs) || (b.res != nullptr) != (a.res != nullptr) || (b.aux != nullptr) != (a.aux != nullptr) ||
        (b.aux2 != nullptr) != (a.aux2 != nullptr) || (b.y2 != nullptr) != (a.y2 != nullptr) ||
        (b.bias != nullptr) != (a.bias != nullptr) || (b.xv != nullptr) != (a.xv != nullptr))
      return ICM_ERR_ARG;
  }
  return (a.algo == ICM_ALGO_WINOGRAD || a.algo == ICM_ALGO_DIRECT) ? ICM_OK : ICM_ERR_ARG;
}

// floats of one tap class in a packed weight buffer whose (chunk, tap) steps hold ncot 32-row tiles
static long long class_packed_floats(int Cin, int ntaps, int ncot) { return (long long)cdiv(Cin, 8) * ntaps * ncot * 256; }

static bool x_aligned16(const icm_conv_args* arr, int ngroups) {
  bool ok = true;
  for (int gi = 0; gi < ngroups; ++gi) ok = ok && (reinterpret_cast<uintptr_t>(arr[gi].x) & 15) == 0;
  return ok;
}

static int conv_run_grouped(const icm_conv_args* arr, int ngroups, hipStream_t stream) {
  if (int rc = check_group(arr, ngroups)) return rc;
  const icm_conv_args& a = arr[0];
  if (a.algo == ICM_ALGO_WINOGRAD) return run_conv_wino(arr, ngroups, stream);
  const int S_in = a.transposed ? 1 : a.stride, out_s = a.transposed ? a.stride : 1;
  long long off = 0;
  for (const ConvClass& cls : build_classes(a.KH, a.KW, a.stride, a.pad, a.transposed)) {
    ConvPlan p;
    int rc = plan_class(a, ngroups, cls, S_in, out_s, x_aligned16(arr, ngroups), p);
    if (!rc) rc = launch_class(arr, ngroups, cls, off, S_in, out_s, p, stream);
    if (rc) return rc;
    off += class_packed_floats(a.Cin, (int)cls.taps.size(), cdiv(a.Cout, 32));
  }
  return ICM_OK;
}

static PackDesc make_pack_desc(const icm_pack_job& J, const ConvClass& cls, long long off) {
  const int ntaps = (int)cls.taps.size(), ncot = cdiv(J.Cout, 32);
  PackDesc d{};
  d.w = J.w;
  d.wp = J.wp + off;
  d.Co = J.Cout; d.Ci = J.Cin; d.KHW = J.KH * J.KW; d.src_out_major = J.src_out_major;
  d.ntaps = ntaps; d.ncot = ncot; d.nchunks = cdiv(J.Cin, 8); d.nonneg = J.nonneg;
  d.bound = J.bound; d.pedestal = J.pedestal;
  d.src_ld = J.src_ld > 0 ? J.src_ld : (J.src_out_major ? J.Cin : J.Cout); d.src_off = J.src_off;
  d.dst_ncot = J.dst_ncot > 0 ? J.dst_ncot : ncot; d.dst_cot_off = J.dst_cot_off; d.wino = J.wino;
  d.cg = d.KHW == 1 ? 4 : 1;   // a 1x1 weight's item spans 32 input channels: 128-byte source rows in either layout
  d.ngroups = cdiv(d.nchunks, d.cg);
  // first float of a row = (outer * src_ld + src_off + a multiple of 8) * KHW
  d.vec = (reinterpret_cast<uintptr_t>(J.w) & 15) == 0 && ((long long)d.src_ld * d.KHW) % 4 == 0 &&
          ((long long)d.src_off * d.KHW) % 4 == 0;
  for (int t = 0; t < ntaps; ++t) d.tapidx[t] = (short)cls.taps[t].kidx;
  return d;
}
static int pack_items(const PackDesc& d) { return d.ncot * d.ngroups; }
static size_t pack_lds_bytes(const PackDesc& d) { return sizeof(float) * pack_lds_floats(d.cg, d.KHW); }

}  // namespace icm

extern "C" {

int icm_conv_run(const icm_conv_args* a, void* stream) {
  return icm::conv_run_grouped(a, 1, (hipStream_t)stream);
}
int icm_conv_run_grouped(const icm_conv_args* a, int ngroups, void* stream) {
  return icm::conv_run_grouped(a, ngroups, (hipStream_t)stream);
}
int icm_conv2d_fwd(const icm_conv_args* a, void* stream) {
  if (!a || a->transposed) return ICM_ERR_ARG;
  return icm_conv_run(a, stream);
}
int icm_convT2d_dgrad(const icm_conv_args* a, void* stream) {
  if (!a || a->transposed) return ICM_ERR_ARG;
  return icm_conv_run(a, stream);
}
int icm_conv2d_dgrad(const icm_conv_args* a, void* stream) {
  if (!a || !a->transposed) return ICM_ERR_ARG;
  return icm_conv_run(a, stream);
}
int icm_convT2d_fwd(const icm_conv_args* a, void* stream) {
  if (!a || !a->transposed) return ICM_ERR_ARG;
  return icm_conv_run(a, stream);
}

int icm_conv_winograd_ok(const icm_conv_args* a) { return (a && icm::wino_supported(*a)) ? 1 : 0; }
int64_t icm_wino_transform_floats(const icm_conv_args* a) {
  return (a && icm::wino_supported(*a) && a->N > 0 && a->Cin > 0) ? (int64_t)icm::wino_transform_floats(*a) : -1;
}
int icm_wino_transform(const icm_conv_args* arr, int ngroups, void* stream) {
  if (!arr || ngroups < 1 || ngroups > ICM_MAX_GROUPS) return ICM_ERR_ARG;
  for (int i = 1; i < ngroups; ++i)
    if (arr[i].N != arr[0].N || arr[i].Cin != arr[0].Cin || arr[i].H != arr[0].H || arr[i].W != arr[0].W ||
        arr[i].x_bs != arr[0].x_bs || arr[i].pro_act != arr[0].pro_act || arr[i].x_seg_len != arr[0].x_seg_len ||
        arr[i].x_seg_gap != arr[0].x_seg_gap)
      return ICM_ERR_ARG;
  return icm::run_wino_transform(arr, ngroups, (hipStream_t)stream);
}

void icm_debug_force_conv_cfg(int idx) { icm::g_force_cfg = idx < 0 ? ICM_CONV_CFG_AUTO : idx; }
int icm_debug_forced_conv_cfg(void) { return icm::g_force_cfg; }
void icm_debug_force_conv1x1(int mode) { icm::g_force_1x1 = mode; }

int icm_debug_conv_plan(const icm_conv_args* arr, int ngroups, int cls, int64_t out[16]) {
  using namespace icm;
  std::fill(out, out + 16, 0);
  int rc = check_group(arr, ngroups);
  if (rc) return rc;
  const icm_conv_args& a = arr[0];
  if (a.algo == ICM_ALGO_WINOGRAD) {
    WinoPlan w{};
    if (cls != 0) return ICM_ERR_ARG;
    if ((rc = plan_conv_wino(a, ngroups, w))) return rc;
    const int64_t v[13] = {1, w.w8 ? kFamWino8 : kFamWino44, w.tco, w.g.lgTX, w.g.lgTY, w.g.lgTI, w.g.nsteps, w.ncb, w.nblk,
                           (int64_t)w.lds_bytes, 512, a.xv != nullptr, w.px_fast};
    std::copy(v, v + 13, out);
    return ICM_OK;
  }
  const std::vector<ConvClass> classes = build_classes(a.KH, a.KW, a.stride, a.pad, a.transposed);
  if (cls < 0 || cls >= (int)classes.size()) return ICM_ERR_ARG;
  long long off = 0;
  for (int i = 0; i < cls; ++i) off += class_packed_floats(a.Cin, (int)classes[i].taps.size(), cdiv(a.Cout, 32));
  ConvPlan p;
  rc = plan_class(a, ngroups, classes[cls], a.transposed ? 1 : a.stride, a.transposed ? a.stride : 1, x_aligned16(arr, ngroups), p);
  if (rc) return rc;
  const int64_t v[14] = {(int64_t)classes.size(), p.family, p.row, p.g.lgTW, p.g.lgTH, p.g.lgTI, p.g.ckm, p.ncb, p.nblk,
                         (int64_t)p.g.lds_bytes, p.block, p.vec4, p.dma, off};
  std::copy(v, v + 14, out);
  return ICM_OK;
}

int64_t icm_packed_weight_floats(int Cout, int Cin, int KH, int KW) {
  return icm::class_packed_floats(Cin, KH * KW, icm::cdiv(Cout, 32));
}

int icm_pack_weights(const float* w, float* wp, int Cout, int Cin, int KH, int KW, int src_out_major,
                     int transposed, int stride, int pad, int nonneg, float bound, float pedestal, void* stream) {
  using namespace icm;
  if (!w || !wp || Cout <= 0 || Cin <= 0 || KH * KW > ICM_MAX_TAPS || (stride != 1 && stride != 2)) return ICM_ERR_ARG;
  icm_pack_job J{};   // natural source row length and destination tiling, spatial taps
  J.w = w; J.wp = wp; J.Cout = Cout; J.Cin = Cin; J.KH = KH; J.KW = KW; J.src_out_major = src_out_major; J.nonneg = nonneg;
  J.bound = bound; J.pedestal = pedestal;
  long long off = 0;
  for (const ConvClass& cls : build_classes(KH, KW, stride, pad, transposed)) {
    if (cls.taps.empty()) continue;
    const PackDesc d = make_pack_desc(J, cls, off);
    hipLaunchKernelGGL(pack_weights_kernel, dim3(pack_items(d)), dim3(256), pack_lds_bytes(d), (hipStream_t)stream, d);
    ICM_CHECK_LAUNCH();
    off += class_packed_floats(Cin, d.ntaps, d.dst_ncot);
  }
  return ICM_OK;
}

int icm_pack_weights_batch(const icm_pack_job* jobs, int n, void* stream) {
  using namespace icm;
  if (!jobs || n < 1) return ICM_ERR_ARG;
  PackMulti m{};
  int nb = 0;
  auto flush = [&]() -> int {
    if (nb == 0) return ICM_OK;
    long long items = 0;
    size_t lds = 0;
    for (int i = 0; i < ICM_PACK_NB; ++i) {
      m.first[i] = i < nb ? (int)items : INT_MAX;
      if (i >= nb) continue;
      items += pack_items(m.g[i]);
      lds = std::max(lds, pack_lds_bytes(m.g[i]));
    }
    if (items > INT_MAX) return ICM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(pack_weights_multi_kernel, dim3((unsigned)items), dim3(256), lds, (hipStream_t)stream, m);
    ICM_CHECK_LAUNCH();
    nb = 0;
    return ICM_OK;
  };
  for (int k = 0; k < n; ++k) {
    const icm_pack_job& J = jobs[k];
    if (!J.w || !J.wp || J.Cout <= 0 || J.Cin <= 0 || J.KH * J.KW > ICM_MAX_TAPS || (J.stride != 1 && J.stride != 2))
      return ICM_ERR_ARG;
    std::vector<ConvClass> classes = build_classes(J.KH, J.KW, J.stride, J.pad, J.transposed);
    if (J.wino) {   // Winograd-domain weights of a 3x3 stride-1 kernel: one "class" of 16 transform points
      if (J.wino < 0 || J.wino > 2 || J.KH != 3 || J.KW != 3 || J.stride != 1 || J.pad != 1 || J.nonneg) return ICM_ERR_ARG;
      ConvClass wc;
      wc.cy = wc.cx = wc.iy0 = wc.ix0 = 0;
      wc.ey = wc.ex = 1;
      for (int t = 0; t < 16; ++t) wc.taps.push_back({0, 0, 0});
      classes.assign(1, wc);
    }
    const int ncot = cdiv(J.Cout, 32), inner = J.src_out_major ? J.Cin : J.Cout;
    if (J.src_off < 0 || J.src_off + inner > (J.src_ld > 0 ? J.src_ld : inner) || J.dst_cot_off < 0 ||
        J.dst_cot_off + ncot > (J.dst_ncot > 0 ? J.dst_ncot : ncot))
      return ICM_ERR_ARG;
    long long off = 0;
    for (const ConvClass& cls : classes) {
      if (cls.taps.empty()) continue;
      const PackDesc& d = m.g[nb] = make_pack_desc(J, cls, off);
      off += class_packed_floats(J.Cin, d.ntaps, d.dst_ncot);   // class stride of the (possibly concatenated) destination
      if (++nb == ICM_PACK_NB) {
        int rc = flush();
        if (rc) return rc;
      }
    }
  }
  return flush();
}

}  // extern "C"
