// Lane streams on the device: the kernels behind compress(coder="lanes") / decompress(coder="lanes").
//
// Format and state machine: icm_amd/bitstream.py ("lane stream"); executable definition: csrc/rans_lanes_common.h (the
// arithmetic of a lane's step, compiled here and into the host coder alike) plus the host loops of csrc/rans.cpp
// (icm_rans_lanes_encode / icm_rans_lanes_decoder_*), which these kernels match byte for byte.  What is this file's
// own: the word order inside a phase and the CDF search.  Parity unpinned: no counterpart in the reference.
//
// One wave codes one body.  A lane owns one 32-bit rANS state; in step t of a run, lane l of wave g handles element
// g c + 64 t + l.  The only cross-lane traffic is the word order inside a phase: the lanes that renormalise take
// consecutive words in ascending lane order = a 64-bit ballot and a popcount of the lower lanes (v_mbcnt), no LDS.
// The word cursor is wave-uniform and lives in a scalar register between steps.
//
// Ranges.  Bodies share nothing, so the decoder's two kernels take a range of waves [g0, g1): the grid holds those waves
// alone (g = g0 + the wave's place in the grid, a scalar), the caller's indexes / out begin at element elem0 <= g0 c of
// the run, and state, cursor and status of every other wave are neither read nor written.  The whole-run entries are
// the range (0, G) from element 0.  A region decode of the residual layer is the user (icm_amd/residual.py).
//
// Bounds.  Every loop is counted by the run length and G (steps), by the constant 3 (escape phases) or by
// ceil(log2(cdf_stride)) (table search); nothing in a stream can lengthen one.  Every word read is checked against
// the body's word count first and sets ICM_LANES_ST_OVERRUN instead of reading; every CDF index is checked against
// ncdf and its table size against the stride before a table entry is read; the search keeps 0 <= lo < hi <= size - 1.
// The encoder checks every word position against its scratch region and sets an overflow flag instead of writing.
#include "icm_common.h"
#include "rans_lanes_common.h"

#include <cstring>
#include <new>
#include <vector>

namespace {

using namespace icm::lanes;

constexpr int kBlock = 256;   // pack / init / finish launches; upper bound of a coding workgroup
constexpr int kEncBad = 1, kEncOverflow = 2;   // flags of the encoder's result record

struct Tab : Tables {
  int maxit;                  // probes that bound the CDF search: ceil(log2(stride)) + 1
};

struct EncResult {   // first 16 bytes of the encoder workspace
  int64_t nbytes;
  int32_t flags, pad;
};

struct WaveCtl {     // decoder: one per body
  uint32_t off;      // byte offset of the body's first word (after its 64 states) inside the uploaded string
  uint32_t nwords;
  uint32_t cursor;
  uint32_t status;
};

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & (kLanes - 1)); }
__device__ __forceinline__ int rank_below(unsigned long long mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
__device__ __forceinline__ int wave_or(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------------ encoder
__global__ void lanes_enc_init_kernel(uint32_t* __restrict__ states, int32_t* __restrict__ wptr, EncResult* res, int G,
                                      int cap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < G * kLanes) states[i] = kL;
  if (i < G) wptr[i] = cap;
  if (i == 0) { res->nbytes = 0; res->flags = 0; res->pad = 0; }
}

// one run, walked last step to first; the words go downwards into this wave's scratch region [0, cap)
__global__ __launch_bounds__(kBlock) void lanes_enc_run_kernel(const int32_t* __restrict__ symbols,
                                                               const int32_t* __restrict__ indexes, long long n,
                                                               long long c, Tab T, uint32_t* __restrict__ states,
                                                               int32_t* __restrict__ wptr, uint16_t* __restrict__ scratch,
                                                               int cap, EncResult* res, int G) {
  const int g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x / kLanes) + threadIdx.x / kLanes));
  if (g >= G) return;
  const int lane = lane_id();
  const long long e0 = (long long)g * c;
  const long long e1 = min(n, e0 + c);
  if (e1 <= e0) return;
  const int steps = (int)((e1 - e0 + kLanes - 1) / kLanes);
  uint32_t x = states[g * kLanes + lane];
  int wp = __builtin_amdgcn_readfirstlane(wptr[g]);
  uint16_t* out = scratch + (long long)g * cap;
  int flags = 0;
  for (int t = steps - 1; t >= 0; --t) {
    const long long e = e0 + (long long)t * kLanes + lane;
    const bool active = e < e1;
    Puts p = {};
    bool ok = false;
    if (active) {
      const int idx = indexes[e], size = ICM_LANES_SIZE(T, idx);
      if (ICM_LANES_FITS(T, size)) ok = plan(T, idx, size, symbols[e], p);
      if (!ok) { flags |= kEncBad; p.esc = false; }
    }
#pragma unroll
    for (int ph = 3; ph >= 0; --ph) {
      const bool puts = ok && p.has(ph);
      const uint32_t f = p.freq(ph), s = p.start(ph);
      const bool emit = puts && put_emits(x, f);
      const unsigned long long mask = __ballot(emit);
      if (mask == 0 && !__any(puts)) continue;
      wp -= __popcll(mask);
      if (emit) {
        const int pos = wp + rank_below(mask);
        if (pos >= 0) out[pos] = (uint16_t)(x & 0xFFFF);
        else flags |= kEncOverflow;
        x >>= 16;
      }
      if (puts) x = put(x, s, f);
    }
  }
  states[g * kLanes + lane] = x;
  if (lane == 0) wptr[g] = wp;
  flags = wave_or(flags);
  if (lane == 0 && flags) atomicOr(&res->flags, flags);
}

// body g -> its place in the string; block g adds up the lengths before it (G <= 4096), the last block writes the total
__global__ __launch_bounds__(kBlock) void lanes_pack_kernel(const uint32_t* __restrict__ states,
                                                            const int32_t* __restrict__ wptr,
                                                            const uint16_t* __restrict__ scratch, int cap, int G,
                                                            uint8_t* __restrict__ out, EncResult* res) {
  __shared__ long long part[kBlock];
  const int g = blockIdx.x, tid = threadIdx.x;
  long long sum = 0;
  for (int k = tid; k < g; k += kBlock) sum += 4 * kLanes + 2ll * (cap - max(wptr[k], 0));
  part[tid] = sum;
  __syncthreads();
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  const int wp = max(wptr[g], 0);
  const int nwords = cap - wp;
  const long long off = 8 + 4ll * G + part[0];
  const uint32_t len = (uint32_t)(4 * kLanes + 2 * nwords);
  uint16_t* o16 = reinterpret_cast<uint16_t*>(out);   // every offset below is even
  if (tid == 0) {
    if (g == 0) {
      out[0] = 'I'; out[1] = 'C'; out[2] = 'M'; out[3] = 'L';
      o16[2] = 1;
      o16[3] = (uint16_t)G;
    }
    o16[4 + 2 * g] = (uint16_t)(len & 0xFFFF);
    o16[5 + 2 * g] = (uint16_t)(len >> 16);
    if (g == G - 1) res->nbytes = off + len;
  }
  uint16_t* body = o16 + off / 2;
  if (tid < kLanes) {
    const uint32_t x = states[g * kLanes + tid];
    body[2 * tid] = (uint16_t)(x & 0xFFFF);
    body[2 * tid + 1] = (uint16_t)(x >> 16);
  }
  const uint16_t* src = scratch + (long long)g * cap + wp;
  for (int k = tid; k < nwords; k += kBlock) body[2 * kLanes + k] = src[k];
}

// ------------------------------------------------------------------------------------------------------ decoder
// s with cdf[s] <= cum < cdf[s + 1], for a table with cdf[0] = 0 and cdf[size - 1] = 2^16 (any other table still ends
// with 0 <= s <= size - 2 after at most 2 maxit probes).  CENTRE: gallop outward from the bin of symbol 0 first --
// nearly every symbol of a Gaussian table lies a few bins from it, but a wave pays for its farthest lane, in both
// directions of the divergent gallop: measured slower than the plain search, kept as a measurement switch.
template <bool CENTRE>
__device__ __forceinline__ int cdf_search(const int32_t* __restrict__ cdf, int size, int centre, int cum, int maxit) {
  int lo = 0, hi = size - 1;
  if (CENTRE) {
    const int c = min(max(centre, 0), size - 2);
    if (cdf[c] <= cum) {
      lo = c;
      int step = 1;
      for (int it = 0; it < maxit; ++it) {
        const int p = lo + step;
        if (p >= hi) break;
        if (cdf[p] <= cum) { lo = p; step <<= 1; }
        else { hi = p; break; }
      }
    } else {
      hi = c;
      int step = 1;
      for (int it = 0; it < maxit; ++it) {
        const int p = hi - step;
        if (p <= lo) break;
        if (cdf[p] > cum) { hi = p; step <<= 1; }
        else { lo = p; break; }
      }
    }
  }
  for (int it = 0; it < maxit && hi - lo > 1; ++it) {
    const int mid = (lo + hi) >> 1;
    if (cdf[mid] <= cum) lo = mid;
    else hi = mid;
  }
  return lo;
}

template <bool CENTRE>
__global__ __launch_bounds__(kBlock) void lanes_dec_run_kernel(const uint8_t* __restrict__ string, WaveCtl* __restrict__ ctl,
                                                               uint32_t* __restrict__ states,
                                                               const int32_t* __restrict__ indexes, long long n,
                                                               long long c, Tab T, int32_t* __restrict__ out, int g0,
                                                               int g1, long long elem0) {
  // the grid holds the waves g0 .. g1 - 1 alone; g0 is a kernel argument, so g stays a scalar
  const int g = g0 + __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x / kLanes) + threadIdx.x / kLanes));
  if (g >= g1) return;
  const int lane = lane_id();
  const long long e0 = (long long)g * c;
  const long long e1 = min(n, e0 + c);
  if (e1 <= e0) return;
  const int steps = (int)((e1 - e0 + kLanes - 1) / kLanes);
  indexes -= elem0;   // the caller's buffers begin at element elem0 <= g0 c <= e0: element e lies at [e] again
  out -= elem0;
  const uint16_t* __restrict__ words = reinterpret_cast<const uint16_t*>(string + ctl[g].off);
  const uint32_t nwords = __builtin_amdgcn_readfirstlane(ctl[g].nwords);
  uint32_t cur = __builtin_amdgcn_readfirstlane(ctl[g].cursor);
  uint32_t x = states[g * kLanes + lane];
  int st = 0;
  for (int t = 0; t < steps; ++t) {
    const long long e = e0 + (long long)t * kLanes + lane;
    const bool active = e < e1;
    bool ok = false, esc = false;
    int sym = 0, overflow = 0, offset = 0;
    if (active) {
      const int idx = indexes[e], size = ICM_LANES_SIZE(T, idx);
      if (ICM_LANES_FITS(T, size)) {
        const int32_t* cdf = T.cdfs + (long long)idx * T.stride;
        offset = T.offsets[idx];
        overflow = size - 2;
        const int cum = (int)(x & 0xFFFF);
        const int s = cdf_search<CENTRE>(cdf, size, -offset, cum, T.maxit);
        const int lo = cdf[s], hi = cdf[s + 1];
        if (in_bin(cum, lo, hi)) {
          ok = true;
          x = advance(x, cum, lo, hi);
          esc = s == overflow;
          sym = s + offset;
        } else {
          st |= ICM_LANES_ST_SYMBOL;
        }
      } else {
        st |= ICM_LANES_ST_INDEX;
      }
    }
    {   // phase 0 renormalisation
      const bool need = ok && x < kL;
      const unsigned long long mask = __ballot(need);
      if (need) {
        const uint32_t k = cur + (uint32_t)rank_below(mask);
        uint32_t w = 0;
        if (k < nwords) w = words[k];
        else st |= ICM_LANES_ST_OVERRUN;
        x = (x << 16) | w;
      }
      cur += (uint32_t)__popcll(mask);
    }
    const unsigned long long emask = __ballot(esc);
    if (emask) {   // wave-uniform: phases 1..3, raw 16-bit groups of the lanes that escaped
      unsigned long long raw = 0;
      const int cnt = __popcll(emask);
#pragma unroll
      for (int ph = 0; ph < 3; ++ph) {
        if (esc) {
          raw |= (unsigned long long)(x & 0xFFFF) << (16 * ph);
          const uint32_t k = cur + (uint32_t)rank_below(emask);
          uint32_t w = 0;
          if (k < nwords) w = words[k];
          else st |= ICM_LANES_ST_OVERRUN;
          x = (x & 0xFFFF0000u) | w;
        }
        cur += (uint32_t)cnt;
      }
      if (esc) {
        const long long v = unescape(raw, overflow, offset);
        if (!is_int32(v)) { st |= ICM_LANES_ST_ESCAPE; sym = 0; }
        else sym = (int)v;
      }
    }
    if (active) out[e] = sym;
  }
  states[g * kLanes + lane] = x;
  st = wave_or(st);
  if (lane == 0) {
    ctl[g].cursor = cur;
    if (st) ctl[g].status |= (uint32_t)st;
  }
}

// the status word of the waves g0 .. g1 - 1; end: with the checks of a body that has decoded its last run
__global__ void lanes_dec_finish_kernel(const WaveCtl* __restrict__ ctl, const uint32_t* __restrict__ states,
                                        uint32_t* __restrict__ status, int g0, int g1, int end) {
  const int g = g0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= g1) return;
  uint32_t st = ctl[g].status;
  if (end) {
    if (ctl[g].cursor != ctl[g].nwords) st |= ICM_LANES_ST_CURSOR;
    for (int l = 0; l < kLanes; ++l)
      if (states[g * kLanes + l] != kL) st |= ICM_LANES_ST_STATE;
  }
  status[g] = st;
}

// ------------------------------------------------------------------------------------------------------ host side
inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

struct EncPlan {
  int G = 0;
  int64_t cap = 0;        // u16 words of scratch per wave
  int64_t o_states, o_wptr, o_scratch, o_out, bytes;
};

bool enc_plan(const int64_t* run_lengths, int nruns, int64_t spw, int worst, EncPlan& P) {
  P.G = icm_rans_lanes_waves(run_lengths, nruns, spw);
  if (P.G < 1) return false;
  int64_t sum_c = 0;
  for (int r = 0; r < nruns; ++r) sum_c += chunk(run_lengths[r], P.G);
  P.cap = (worst ? 4 : 1) * sum_c;
  if (P.cap >= (1ll << 29)) return false;           // word positions are 32-bit in the kernels: a wave's pointer starts
                                                    // at cap and falls by at most 4 cap, so it stays above INT32_MIN
  P.o_states = align16((int64_t)sizeof(EncResult));
  P.o_wptr = P.o_states + align16(4ll * P.G * kLanes);
  P.o_scratch = P.o_wptr + align16(4ll * P.G);
  P.o_out = P.o_scratch + align16(2 * P.cap * P.G);
  P.bytes = P.o_out + align16(8 + 4ll * P.G + (int64_t)P.G * (4 * kLanes + 2 * P.cap));
  return true;
}

bool make_tab(const int32_t* cdfs, int stride, const int32_t* sizes, const int32_t* offsets, int ncdf, Tab& T) {
  T = Tab{{cdfs, sizes, offsets, stride, ncdf}, 0};
  if (!T.ok()) return false;
  T.maxit = icm::ceil_log2(stride) + 1;
  return true;
}

struct GpuDecoder {
  std::vector<uint8_t> host;    // what create uploads; kept until destroy (the copy is asynchronous)
  uint8_t* dev = nullptr;
  int G = 0;
  int64_t o_ctl, o_states, o_status, o_string;
  hipStream_t stream = nullptr;   // the stream create uploaded on
};

int g_search_centre = 0;   // binary search: measured 2x faster than centre-first on wide tables

// Waves (bodies) per coding workgroup.  The waves of a stream share nothing, and a stream has few of them (48 per slice
// of a 2048x3072 image), each a serial chain of dependent loads: one wave per workgroup lets the dispatcher spread
// them over as many CUs as there are bodies.  ICM_LANES_WPB (1, 2 or 4) is the measurement knob.
int waves_per_block() {
  static const int w = icm::env_int("ICM_LANES_WPB", 1);
  return w == 2 || w == 4 ? w : 1;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" {

void icm_debug_lanes_search(int centre) { g_search_centre = centre ? 1 : 0; }

int64_t icm_rans_lanes_encode_gpu_workspace(const int64_t* run_lengths, int nruns, int64_t symbols_per_wave,
                                            int worst_case) {
  EncPlan P;
  return enc_plan(run_lengths, nruns, symbols_per_wave, worst_case, P) ? P.bytes : -1;
}

int64_t icm_rans_lanes_encode_gpu(const int32_t* symbols, const int32_t* indexes, const int64_t* run_lengths, int nruns,
                                  const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets,
                                  int ncdf, int64_t symbols_per_wave, int worst_case, void* ws, int64_t ws_bytes,
                                  int64_t* string_offset, void* stream) {
  EncPlan P;
  Tab T;
  if (!enc_plan(run_lengths, nruns, symbols_per_wave, worst_case, P) || !make_tab(cdfs, cdf_stride, cdf_sizes, offsets, ncdf, T))
    return -1;
  int64_t total = 0;
  for (int r = 0; r < nruns; ++r) total += run_lengths[r];
  if ((total > 0 && (!symbols || !indexes)) || !ws || !string_offset || ws_bytes < P.bytes ||
      (reinterpret_cast<uintptr_t>(ws) & 15))
    return -1;
  uint8_t* base = static_cast<uint8_t*>(ws);
  EncResult* res = reinterpret_cast<EncResult*>(base);
  uint32_t* states = reinterpret_cast<uint32_t*>(base + P.o_states);
  int32_t* wptr = reinterpret_cast<int32_t*>(base + P.o_wptr);
  uint16_t* scratch = reinterpret_cast<uint16_t*>(base + P.o_scratch);
  const int G = P.G, cap = (int)P.cap;
  hipLaunchKernelGGL(lanes_enc_init_kernel, dim3((G * kLanes + kBlock - 1) / kBlock), dim3(kBlock), 0, ST, states, wptr,
                     res, G, cap);
  if (hipGetLastError() != hipSuccess) return -3;
  const int wpb = waves_per_block();
  const int blocks = (G + wpb - 1) / wpb;
  int64_t off = total;
  for (int r = nruns - 1; r >= 0; --r) {
    const int64_t n = run_lengths[r];
    off -= n;
    if (n == 0) continue;
    hipLaunchKernelGGL(lanes_enc_run_kernel, dim3(blocks), dim3(wpb * kLanes), 0, ST, symbols + off, indexes + off,
                       (long long)n, (long long)chunk(n, G), T, states, wptr, scratch, cap, res, G);
    if (hipGetLastError() != hipSuccess) return -3;
  }
  hipLaunchKernelGGL(lanes_pack_kernel, dim3(G), dim3(kBlock), 0, ST, states, wptr, scratch, cap, G, base + P.o_out, res);
  if (hipGetLastError() != hipSuccess) return -3;
  EncResult h;
  if (hipMemcpyAsync(&h, res, sizeof(h), hipMemcpyDeviceToHost, ST) != hipSuccess) return -3;
  if (hipStreamSynchronize(ST) != hipSuccess) return -3;
  if (h.flags & kEncBad) return -1;
  if (h.flags & kEncOverflow) return -2;
  *string_offset = P.o_out;
  return h.nbytes;
}

void* icm_rans_lanes_decoder_gpu_create(const uint8_t* stream_bytes, int64_t nbytes, void* stream) {
  if (!stream_bytes || nbytes < 8 || nbytes >= (1ll << 31)) return nullptr;
  GpuDecoder* D = nullptr;
  try {
    std::vector<Body> body;
    if (!parse(stream_bytes, nbytes, body)) return nullptr;   // header and length table, on the host
    D = new GpuDecoder();
    const int G = (int)body.size();
    D->G = G;
    D->stream = ST;
    D->o_ctl = 0;
    D->o_states = align16((int64_t)sizeof(WaveCtl) * G);
    D->o_status = D->o_states + align16(4ll * G * kLanes);
    D->o_string = D->o_status + align16(4ll * G);
    D->host.assign((size_t)(D->o_string + align16(nbytes)), 0);
    WaveCtl* ctl = reinterpret_cast<WaveCtl*>(D->host.data());
    for (int g = 0; g < G; ++g) {
      ctl[g] = WaveCtl{(uint32_t)(D->o_string + body[g].off + kBodyMin), (uint32_t)body[g].words, 0u, 0u};
      std::memcpy(D->host.data() + D->o_states + 4ll * g * kLanes, stream_bytes + body[g].off, kBodyMin);
    }
    std::memcpy(D->host.data() + D->o_string, stream_bytes, (size_t)nbytes);
    if (hipMalloc(reinterpret_cast<void**>(&D->dev), D->host.size()) == hipSuccess &&
        hipMemcpyAsync(D->dev, D->host.data(), D->host.size(), hipMemcpyHostToDevice, ST) == hipSuccess)
      return D;
  } catch (const std::bad_alloc&) {
  }
  icm_rans_lanes_decoder_gpu_destroy(D);
  return nullptr;
}

int icm_rans_lanes_decoder_gpu_decode_run(void* decoder, const int32_t* indexes, int64_t n, const int32_t* cdfs,
                                          int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int ncdf,
                                          int32_t* out, void* stream) {
  if (!decoder) return ICM_ERR_ARG;
  return icm_rans_lanes_decoder_gpu_decode_run_waves(decoder, 0, static_cast<GpuDecoder*>(decoder)->G, 0, indexes, n,
                                                     cdfs, cdf_stride, cdf_sizes, offsets, ncdf, out, stream);
}

int icm_rans_lanes_decoder_gpu_waves(void* decoder) { return decoder ? static_cast<GpuDecoder*>(decoder)->G : -1; }

int icm_rans_lanes_decoder_gpu_decode_run_waves(void* decoder, int g0, int g1, int64_t elem0, const int32_t* indexes,
                                                int64_t n, const int32_t* cdfs, int cdf_stride,
                                                const int32_t* cdf_sizes, const int32_t* offsets, int ncdf,
                                                int32_t* out, void* stream) {
  Tab T;
  if (!decoder || n < 0 || !make_tab(cdfs, cdf_stride, cdf_sizes, offsets, ncdf, T)) return ICM_ERR_ARG;
  GpuDecoder& D = *static_cast<GpuDecoder*>(decoder);
  const int64_t c = chunk(n, D.G);
  if (g0 < 0 || g0 > g1 || g1 > D.G || elem0 < 0 || elem0 > (int64_t)g0 * c) return ICM_ERR_ARG;
  const bool owns = g0 < g1 && (int64_t)g0 * c < n;   // a range that owns no element needs no buffers
  if (owns && (!indexes || !out)) return ICM_ERR_ARG;
  if (!owns) return ICM_OK;
  const int wpb = waves_per_block();
  const int blocks = (g1 - g0 + wpb - 1) / wpb;   // the range's waves alone
  WaveCtl* ctl = reinterpret_cast<WaveCtl*>(D.dev + D.o_ctl);
  uint32_t* states = reinterpret_cast<uint32_t*>(D.dev + D.o_states);
  // the kernel addresses the string from the allocation's base: WaveCtl.off includes o_string
  hipLaunchKernelGGL(g_search_centre ? lanes_dec_run_kernel<true> : lanes_dec_run_kernel<false>, dim3(blocks),
                     dim3(wpb * kLanes), 0, ST, D.dev, ctl, states, indexes, (long long)n, (long long)c, T, out, g0, g1,
                     (long long)elem0);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_rans_lanes_decoder_gpu_finish(void* decoder, void* stream) {
  if (!decoder) return -1;
  return icm_rans_lanes_decoder_gpu_finish_waves(decoder, 0, static_cast<GpuDecoder*>(decoder)->G, 1, stream);
}

int icm_rans_lanes_decoder_gpu_finish_waves(void* decoder, int g0, int g1, int end, void* stream) {
  if (!decoder) return -1;
  GpuDecoder& D = *static_cast<GpuDecoder*>(decoder);
  if (g0 < 0 || g0 > g1 || g1 > D.G) return -1;
  if (g0 == g1) return 0;
  const int ng = g1 - g0;
  uint32_t* status = reinterpret_cast<uint32_t*>(D.dev + D.o_status);
  hipLaunchKernelGGL(lanes_dec_finish_kernel, dim3((ng + kBlock - 1) / kBlock), dim3(kBlock), 0, ST,
                     reinterpret_cast<const WaveCtl*>(D.dev + D.o_ctl),
                     reinterpret_cast<const uint32_t*>(D.dev + D.o_states), status, g0, g1, end ? 1 : 0);
  if (hipGetLastError() != hipSuccess) return -1;
  std::vector<uint32_t> h((size_t)ng);
  if (hipMemcpyAsync(h.data(), status + g0, 4 * (size_t)ng, hipMemcpyDeviceToHost, ST) != hipSuccess) return -1;
  if (hipStreamSynchronize(ST) != hipSuccess) return -1;
  int st = 0;
  for (uint32_t v : h) st |= (int)v;
  return st;
}

void icm_rans_lanes_decoder_gpu_destroy(void* decoder) {
  GpuDecoder* D = static_cast<GpuDecoder*>(decoder);
  if (!D) return;
  if (D->dev) {
    (void)hipStreamSynchronize(D->stream);   // the upload of create reads D->host; the launches read D->dev
    (void)hipFree(D->dev);
  }
  delete D;
}

}  // extern "C"
