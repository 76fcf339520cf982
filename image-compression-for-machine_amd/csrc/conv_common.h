// Shared by the convolution kernels (conv_igemm.hip, conv_1x1.hip, conv_ks8.hip, conv_wino.hip): launch descriptor
// and THE definition of the fused-neighbour epilogue -- what each kind reads and writes (epi_reads_* / epi_writes_side
// / epi_may_gelu), its per-element math (epi_apply, epi_materialise) and the kinds each kernel family is compiled for
// (EpiAll / EpiKs8 / EpiWino: host eligibility test and device dispatch come from the same list).
#pragma once
#include <type_traits>
#include "icm_common.h"

namespace icm {

#define ICM_MAX_TAPS 32
#define ICM_MAX_GROUPS 12   /* problems of identical geometry per launch (blockIdx.y): the independent slice chains */

struct ConvPtrs {
  const float* x;
  const float* wp;
  const float* bias;
  float* y;
  const float* res;
  const float* aux;
  const float* aux2;
  float* y2;
};

struct ConvDesc {
  ConvPtrs g[ICM_MAX_GROUPS];
  long long y_bs, res_bs, aux_bs, aux2_bs, y2_bs;
  PatchGeom pg;                // input tensor + LDS patch layout
  int Cout, OHf, OWf;
  int OHv, OWv;
  int out_sy, out_oy, out_sx, out_ox;
  int iy0, ix0;
  int ntaps;
  int lgTW, lgTH, lgTI;
  int tiles_x, tiles_y, tiles_n;
  int ncot, nchunks8, ckm, ncb;
  int epi, accum, ps2;
  int tapoff[ICM_MAX_TAPS];   // dword entries: read with s_load (a 16-bit entry forces a VMEM load + vmcnt(0))
};

// What every conv kernel family's launch takes straight from the arguments: per-member pointers (unused members repeat
// member 0: every blockIdx.y finds valid pointers), batch strides, GEMM-M size and the epilogue.  d arrives zeroed.
inline void fill_conv_ptrs(ConvPtrs (&g)[ICM_MAX_GROUPS], const icm_conv_args* arr, int ngroups, long long wp_off) {
  for (int gi = 0; gi < ICM_MAX_GROUPS; ++gi) {
    const icm_conv_args& s = arr[gi < ngroups ? gi : 0];
    g[gi] = ConvPtrs{s.x, s.wp + wp_off, s.bias, s.y, s.res, s.aux, s.aux2, s.y2};
  }
}
inline void fill_conv_desc(ConvDesc& d, const icm_conv_args* arr, int ngroups, long long wp_off) {
  const icm_conv_args& a = arr[0];
  fill_conv_ptrs(d.g, arr, ngroups, wp_off);
  d.y_bs = a.y_bs; d.res_bs = a.res_bs; d.aux_bs = a.aux_bs; d.aux2_bs = a.aux2_bs; d.y2_bs = a.y2_bs;
  d.Cout = a.Cout; d.ncot = (a.Cout + 31) / 32;
  d.epi = a.epi; d.accum = a.accum;
}

// ---- launch plans: everything a launch decides, by pure host code, before any HIP call (icm_debug_conv_plan shows them)
enum ConvFamily { kFamStaged = 0, kFamKs8 = 1, kFam1x1 = 2, kFamWino44 = 3, kFamWino8 = 4 };
struct Geometry {   // pixel tile, LDS patch and grid of the LDS-staged kernels
  int lgTW, lgTH, lgTI, PH, PW, PWh, PWrow, PP, CS, tiles_x, tiles_y, tiles_n, ckm;
  size_t lds_bytes;
};
struct ConvPlan {   // one tap class of a direct launch
  int family;       // kFamStaged / kFamKs8 / kFam1x1
  int row;          // row of the family's kernel table (conv_igemm.hip kCfgs, conv_1x1.hip kCfgs1x1); K-split: co tiles per block
  Geometry g;       // the pointwise kernel has none: zeros, ckm = 1
  int ncb;          // co blocks
  long long nblk;   // workgroups per member; 0: nothing to launch
  int block, vec4, dma;
};
struct WinoGeom {
  int lgTX, lgTY, lgTI, tiles_x, tiles_y, tiles_n, nchunks8, nsteps;
};
struct WinoPlan {
  WinoGeom g;
  int tco, w8, px_fast, ncb;   // co tiles per workgroup; 0: the 4 + 4 wave kernel, 1: the eight-MFMA-wave kernel
  long long nblk;
  size_t lds_bytes;
};

// ---- the fused-neighbour epilogue (kinds: include/icm_hip.h): per output element
//   v = acc + bias  ->  epi_apply<EPI>  ->  (+ old y if accum)  ->  epi_materialise (kinds with epi_may_gelu)  ->  y
// Operands of a kind (host validation and the kernels' operand loads both ask these):
constexpr bool epi_reads_res(int e) { return e == ICM_EPI_RES || e == ICM_EPI_RES_GELU || e == ICM_EPI_RES_MUL_DGELU; }
constexpr bool epi_reads_aux(int e) {
  return e == ICM_EPI_GDN || e == ICM_EPI_IGDN || e == ICM_EPI_MUL_DGELU || e == ICM_EPI_AXPY2 || e == ICM_EPI_LRP ||
         e == ICM_EPI_RES_MUL_DGELU;
}
constexpr bool epi_reads_aux2(int e) { return e == ICM_EPI_AXPY2; }
// y2 (when given) receives a side value of epi_apply: the GDN / IGDN norm before the root, the LRP tanh
constexpr bool epi_writes_side(int e) { return e == ICM_EPI_GDN || e == ICM_EPI_IGDN || e == ICM_EPI_LRP; }
// y2 (when given) receives gelu(y): the materialised activation for the consumers of this pre-activation (forward only)
constexpr bool epi_may_gelu(int e) { return e == ICM_EPI_NONE || e == ICM_EPI_RES || e == ICM_EPI_RES_GELU; }

// The math of a kind: v = accumulator + bias, rv = the res operand (AXPY2: the aux2 operand), av = the aux operand;
// returns the value, `side` = what y2 receives for the kinds with epi_writes_side.  Operands a kind does not read are
// ignored.  The callers keep their own load batching, accumulation order and store loops (their register budgets).
template <int EPI>
__device__ __forceinline__ float epi_apply(float v, float rv, float av, float& side) {
  if constexpr (EPI == ICM_EPI_RES) v += rv;
  if constexpr (EPI == ICM_EPI_RES_GELU) v += gelu_f(rv);
  if constexpr (EPI == ICM_EPI_GDN || EPI == ICM_EPI_IGDN) {
    side = v;
    v = av * (EPI == ICM_EPI_GDN ? rsqrtf(v) : sqrtf(v));
  }
  if constexpr (EPI == ICM_EPI_MUL_DGELU) v *= dgelu_f(av);
  if constexpr (EPI == ICM_EPI_RES_MUL_DGELU) v = (v + rv) * dgelu_f(av);
  if constexpr (EPI == ICM_EPI_AXPY2) v = rv + 2.0f * av * v;
  if constexpr (EPI == ICM_EPI_LRP) {
    side = tanhf(v);
    v = av + 0.5f * side;
  }
  return v;
}
// GELU materialisation of the value AFTER an accumulation (the launch that completes a partial sum materialises it);
// y2 must be non-null.  v is what goes to y: with y2 == y (inference: nobody reads the pre-activation again) only
// gelu(v) is stored, so v becomes it; otherwise y2[off] = gelu(v) and y keeps v.
template <class Off>
__device__ __forceinline__ void epi_materialise(float& v, const float* y, float* y2, Off off, bool ok) {
  const float gv = gelu_f(v);
  if (y2 == y) v = gv;
  else if (ok) y2[off] = gv;
}

// The kinds a kernel family is compiled for, named once: has() is the host's eligibility test, dispatch() the device's
// uniform branch -- f(std::integral_constant<int, K>{}) for the matching kind, the ICM_EPI_NONE instantiation for
// anything else.  A kind outside the list costs no code object; a kind inside it is both accepted and instantiated.
template <int... Kinds>
struct EpiKinds {
  static constexpr bool has(int epi) { return ((epi == Kinds) || ...); }
  template <class F>
  static __device__ __forceinline__ void dispatch(int epi, F&& f) {
    static_assert(((Kinds == ICM_EPI_NONE) || ...), "ICM_EPI_NONE is the fallback of every kernel");
    const bool hit = ((Kinds != ICM_EPI_NONE && epi == Kinds ? (f(std::integral_constant<int, Kinds>{}), true) : false) || ...);
    if (!hit) f(std::integral_constant<int, ICM_EPI_NONE>{});
  }
};
// LDS-staged (conv_igemm.hip) and direct 1x1 (conv_1x1.hip) kernels: every kind
using EpiAll = EpiKinds<ICM_EPI_NONE, ICM_EPI_RES, ICM_EPI_RES_GELU, ICM_EPI_GDN, ICM_EPI_IGDN, ICM_EPI_MUL_DGELU,
                        ICM_EPI_AXPY2, ICM_EPI_LRP, ICM_EPI_RES_MUL_DGELU>;
// 8-wave K-split kernel (conv_ks8.hip): GDN / IGDN / AXPY2 belong to pointwise launches, which never take it
using EpiKs8 = EpiKinds<ICM_EPI_NONE, ICM_EPI_RES, ICM_EPI_RES_GELU, ICM_EPI_MUL_DGELU, ICM_EPI_LRP, ICM_EPI_RES_MUL_DGELU>;
// Winograd kernels (conv_wino.hip): the neighbours of the 3x3 stride-1 layers
using EpiWino = EpiKinds<ICM_EPI_NONE, ICM_EPI_RES, ICM_EPI_RES_GELU, ICM_EPI_MUL_DGELU, ICM_EPI_RES_MUL_DGELU, ICM_EPI_LRP>;

// Epilogue of one 32x32 accumulator tile.  The fused-neighbour kind is a template parameter so that the 16 rows
// form ONE basic block: all operand loads (bias, residual, aux, old value) are issued back to back and waited for
// once, instead of a load -> wait -> store chain per element.
template <int EPI, int half>
__device__ __forceinline__ void store_half_e(const ConvDesc& d, const ConvPtrs& P, const f32x16 acc, int cot, int h,
                                             int n, int oy, int ox, bool pvalid) {
  const int plane = d.OHf * d.OWf;
  constexpr bool kRes = epi_reads_res(EPI), kAux = epi_reads_aux(EPI), kAux2 = epi_reads_aux2(EPI);
  float* yb = P.y + n * d.y_bs;
  const float* resb = kRes ? P.res + n * d.res_bs : nullptr;
  const float* auxb = kAux ? P.aux + n * d.aux_bs : nullptr;
  const float* aux2b = kAux2 ? P.aux2 + n * d.aux2_bs : nullptr;
  float* y2b = P.y2 ? P.y2 + n * d.y2_bs : nullptr;
  const bool has_bias = P.bias != nullptr;
  // rows in two halves of 8: bounds the live registers of the load batch (the kernel's VGPR budget sets occupancy)
  {
    int off[8];
    bool ok[8];
    float bv[8], rv[8], av[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int r = half * 8 + q;
      const int co = cot * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      ok[q] = pvalid && co < d.Cout;
      off[q] = d.ps2 ? (co >> 2) * plane + (oy * 2 + ((co >> 1) & 1)) * d.OWf + ox * 2 + (co & 1)
                     : co * plane + oy * d.OWf + ox;
      bv[q] = (has_bias && ok[q]) ? P.bias[co] : 0.0f;
      if constexpr (kRes) rv[q] = ok[q] ? resb[off[q]] : 0.0f;
      if constexpr (kAux) av[q] = ok[q] ? auxb[off[q]] : 0.0f;
      if constexpr (kAux2) rv[q] = ok[q] ? aux2b[off[q]] : 0.0f;
    }
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      float side;
      v[q] = epi_apply<EPI>(acc[half * 8 + q] + bv[q], (kRes || kAux2) ? rv[q] : 0.0f, kAux ? av[q] : 0.0f, side);
      if constexpr (epi_writes_side(EPI))
        if (y2b && ok[q]) y2b[off[q]] = side;
    }
    if (d.accum) {   // accumulation (gradients; partial first-layer sums of the slice chains): one more batched read
      float old[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) old[q] = ok[q] ? yb[off[q]] : 0.0f;
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] += old[q];
    }
    if constexpr (epi_may_gelu(EPI)) {
      if (y2b) {
#pragma unroll
        for (int q = 0; q < 8; ++q) epi_materialise(v[q], yb, y2b, off[q], ok[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (ok[q]) yb[off[q]] = v[q];
  }
}
template <int EPI>
__device__ __forceinline__ void store_tile_e(const ConvDesc& d, const ConvPtrs& P, const f32x16 acc, int cot, int h,
                                             int n, int oy, int ox, bool pvalid) {
  store_half_e<EPI, 0>(d, P, acc, cot, h, n, oy, ox, pvalid);
  store_half_e<EPI, 1>(d, P, acc, cot, h, n, oy, ox, pvalid);
}

// Pipelined form: epilogue of half a 32x32 accumulator tile (8 rows of one lane's column), in two phases so that the callers can
// software-pipeline it: epi_load issues every operand load of the half tile (bias, residual, aux, old value for
// gradient accumulation) back to back; epi_finish consumes them and stores.  The callers issue the loads of half
// tile i+1 BEFORE finishing half tile i: one exposed memory round trip per wave instead of one per half tile (a
// 192 x 32 strip with a residual operand used to pay 12 dependent load -> use -> store round trips).  The fused-
// neighbour kind is a template parameter: each phase is one basic block.
struct EpiRegs {
  int n;
  int off[8];
  bool ok[8];
  float bv[8], rv[8], av[8], old[8];
};

template <int EPI>
__device__ __forceinline__ void epi_load(const ConvDesc& d, const ConvPtrs& P, int cot, int half, int h, int n, int oy,
                                         int ox, bool pvalid, EpiRegs& R) {
  const int plane = d.OHf * d.OWf;
  constexpr bool kRes = epi_reads_res(EPI), kAux = epi_reads_aux(EPI), kAux2 = epi_reads_aux2(EPI);
  const float* yb = P.y + n * d.y_bs;
  const float* resb = kRes ? P.res + n * d.res_bs : nullptr;
  const float* auxb = kAux ? P.aux + n * d.aux_bs : nullptr;
  const float* aux2b = kAux2 ? P.aux2 + n * d.aux2_bs : nullptr;
  const bool has_bias = P.bias != nullptr;
  const bool tile_ok = pvalid && cot < d.ncot;
  R.n = n;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int r = half * 8 + q;
    const int co = cot * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
    R.ok[q] = tile_ok && co < d.Cout;
    R.off[q] = d.ps2 ? (co >> 2) * plane + (oy * 2 + ((co >> 1) & 1)) * d.OWf + ox * 2 + (co & 1)
                     : co * plane + oy * d.OWf + ox;
    R.bv[q] = (has_bias && R.ok[q]) ? P.bias[co] : 0.0f;
    if constexpr (kRes) R.rv[q] = R.ok[q] ? resb[R.off[q]] : 0.0f;
    if constexpr (kAux) R.av[q] = R.ok[q] ? auxb[R.off[q]] : 0.0f;
    if constexpr (kAux2) R.rv[q] = R.ok[q] ? aux2b[R.off[q]] : 0.0f;
  }
  if (d.accum) {   // gradient accumulation: one more batched read of the destination
#pragma unroll
    for (int q = 0; q < 8; ++q) R.old[q] = R.ok[q] ? yb[R.off[q]] : 0.0f;
  }
}

template <int EPI>
__device__ __forceinline__ void epi_finish(const ConvDesc& d, const ConvPtrs& P, const float (&a8)[8], const EpiRegs& R) {
  float* yb = P.y + R.n * d.y_bs;
  float* y2b = P.y2 ? P.y2 + R.n * d.y2_bs : nullptr;
  constexpr bool kRv = epi_reads_res(EPI) || epi_reads_aux2(EPI), kAux = epi_reads_aux(EPI);   // what epi_load filled
  float v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    float side;
    v[q] = epi_apply<EPI>(a8[q] + R.bv[q], kRv ? R.rv[q] : 0.0f, kAux ? R.av[q] : 0.0f, side);
    if constexpr (epi_writes_side(EPI))
      if (y2b && R.ok[q]) y2b[R.off[q]] = side;
  }
  if (d.accum) {
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] += R.old[q];
  }
  if constexpr (epi_may_gelu(EPI)) {
    if (y2b) {
#pragma unroll
      for (int q = 0; q < 8; ++q) epi_materialise(v[q], yb, y2b, R.off[q], R.ok[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < 8; ++q)
    if (R.ok[q]) yb[R.off[q]] = v[q];
}

// All TCO x TPX accumulator tiles of one wave, pipelined over half tiles.  pn / poy / pox / pv: image, output row,
// output column and validity of this lane's pixel in pixel tile tp (a flat 1x1 caller passes row 0, column = offset
// inside the plane).
template <int EPI, int TCO, int TPX, bool PIPE>
__device__ __forceinline__ void epilogue_tiles(const ConvDesc& d, const ConvPtrs& P, const f32x16 (&acc)[TCO][TPX], int cot0,
                                               int h, const int (&pn)[TPX], const int (&poy)[TPX], const int (&pox)[TPX],
                                               const bool (&pv)[TPX]) {
  if constexpr (!PIPE) {
#pragma unroll
    for (int tp = 0; tp < TPX; ++tp)
#pragma unroll
      for (int a = 0; a < TCO; ++a) {
        if (cot0 + a < d.ncot) store_tile_e<EPI>(d, P, acc[a][tp], cot0 + a, h, pn[tp], poy[tp], pox[tp], pv[tp]);
        __builtin_amdgcn_sched_barrier(0);
      }
    return;
  }
  constexpr int S = TPX * TCO * 2;
  EpiRegs R[2];
  epi_load<EPI>(d, P, cot0, 0, h, pn[0], poy[0], pox[0], pv[0], R[0]);
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const int half = i & 1, a = (i >> 1) % TCO, tp = (i >> 1) / TCO;
    if (i + 1 < S) {
      const int i2 = i + 1;
      const int half2 = i2 & 1, a2 = (i2 >> 1) % TCO, tp2 = (i2 >> 1) / TCO;
      epi_load<EPI>(d, P, cot0 + a2, half2, h, pn[tp2], poy[tp2], pox[tp2], pv[tp2], R[i2 & 1]);
    }
    __builtin_amdgcn_sched_barrier(0);
    float a8[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) a8[q] = acc[a][tp][half * 8 + q];
    epi_finish<EPI>(d, P, a8, R[i & 1]);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// the epilogue kind is dispatched ONCE (uniform branch) around the fully unrolled tile loops.  PIPE2: pipeline the
// kinds that read two full-size operands from HBM (AXPY2: x and the dn map of the GDN backward, 2 x 201 MB at
// 128x128 -- measured 0.76 -> 0.54 ms); for the single-operand kinds, whose operand is L2-warm, the extra registers
// of the pipelined form cost more than the round trips (measured), so they keep the batched half-tile form.
template <int TCO, int TPX, bool PIPE2 = false>
__device__ __forceinline__ void epilogue_dispatch(const ConvDesc& d, const ConvPtrs& P, const f32x16 (&acc)[TCO][TPX],
                                                  int cot0, int h, const int (&pn)[TPX], const int (&poy)[TPX],
                                                  const int (&pox)[TPX], const bool (&pv)[TPX]) {
  EpiAll::dispatch(d.epi, [&](auto kind) {
    constexpr int EPI = decltype(kind)::value;
    epilogue_tiles<EPI, TCO, TPX, EPI == ICM_EPI_AXPY2 && PIPE2>(d, P, acc, cot0, h, pn, poy, pox, pv);
  });
}

// latency-bound problems (conv_ks8.hip): eight MFMA waves split K over one block of four tiles (tco = 2: 64 co x 64 px;
// tco = 1: 32 co x 128 px); d must describe a stride-1-sampling, activation-free, linear-patch launch
int launch_conv_ks8(const ConvDesc& d, int tco, long long nblk, int ngroups, size_t lds_bytes, hipStream_t stream);

// Winograd F(2x2, 3x3) path (conv_wino.hip): 3x3 stride-1 pad-1 launches whose weights were packed with wino != 0
bool wino_supported(const icm_conv_args& a);
int plan_conv_wino(const icm_conv_args& a, int ngroups, WinoPlan& p);
int run_conv_wino(const icm_conv_args* arr, int ngroups, hipStream_t stream);
long long wino_transform_floats(const icm_conv_args& a);
int run_wino_transform(const icm_conv_args* arr, int ngroups, hipStream_t stream);

// pointwise path (conv_1x1.hip).  plan: ICM_OK with p filled, -1 when the launch should take the LDS-staged kernel (p
// untouched); launch: d holds what fill_conv_desc and the plan's ncb gave it
int plan_conv1x1(const icm_conv_args& a, int ngroups, int force_mode, ConvPlan& p);
int launch_conv1x1(ConvDesc& d, const icm_conv_args& a, const ConvPlan& p, int ngroups, hipStream_t stream);

}  // namespace icm
