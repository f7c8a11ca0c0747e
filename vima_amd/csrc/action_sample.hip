// Action selection with sampling controls: act_select_kernel (action_select.hip) plus a temperature per row of logits, top-k and
// nucleus (top-p) truncation of every segment, several samples per row of logits, and the scoring of bins the caller already has.
// The semantics (include/vima_hip.h, vima_action_select_ex; fp64 restatement in tests/act_sampling_reference.py):
//
//   z = x / T                      one correctly rounded fp32 division; T clamped to [1e-4, 1e4], a NaN is 1, no T is 1
//   rank(i) = #{j : z_j > z_i} + #{j < i : z_j == z_i}                                     exact comparisons, ties to the lower index
//   top-k:  i survives iff rank(i) < k                                                     (k <= 0 or k >= n: off)
//   top-p:  after top-k, q = softmax(z) over the survivors; the bin of rank r survives iff the mass of the surviving bins of
//           rank < r is < p                                                                (p >= 1: off; rank 0 always survives)
//   pi = softmax(z) over the kept set K, log pi = z - (max z + log sum_K exp(z - max z)) on K, -inf elsewhere
//
// The shape is act_select_kernel's: one 256-thread workgroup per OUTPUT row (row r * S + s is sample s of logits row r), each wave owns
// three of the twelve segments, a lane holds at most two bins, everything is a wave reduction. With every control off the arithmetic
// is act_select_kernel's, operation for operation, so the outputs are bit-identical. The extra work only runs when a filter is on:
// the ranks by a compare loop over the segment's values (lane broadcasts), the rank-ordered cumulative mass of top-p through a
// per-wave LDS array (scatter by rank, two wave scans, gather back) and the second normalisation over K.
// Phase 2 is the first layer of the action embedding from the bins in LDS, as in act_select_kernel.
#include "kernels.h"

namespace vima {

namespace {

constexpr int kSeg = 12;
constexpr int kRankSlots = 128;   // per wave: ranks are < n <= 100

__device__ __forceinline__ int seg_bins(int d) { return (d == 1 || d == 7) ? 100 : 50; }
__device__ __forceinline__ int seg_off(int d) { return 50 * d + (d > 1 ? 50 : 0) + (d > 7 ? 50 : 0); }
__device__ __forceinline__ int key_first(int k) { return k == 0 ? 0 : k == 1 ? 2 : k == 2 ? 6 : 8; }
__device__ __forceinline__ int key_dims(int k) { return (k & 1) ? 4 : 2; }

__device__ __forceinline__ float wave_incl_scan(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
// one wave hands values to its own lanes through LDS: the wave's DS operations execute in order, this keeps the compiler from
// moving them across the hand-off and waits for the stores
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// highest set bit of m at or below position b (b in [0, 64)), or -1
__device__ __forceinline__ int top_bit_at_or_below(unsigned long long m, int b) {
  m &= (b >= 63) ? ~0ull : ((2ull << b) - 1ull);
  return m ? 63 - __clzll((long long)m) : -1;
}

// as in action_select.hip: every operation rounded to fp32 on its own
__device__ __forceinline__ float rescale(float x, float lo, float hi) {
#pragma clang fp contract(off)
  const float span = hi - lo;
  float v = x * span;
  v = v + lo;
  return fminf(fmaxf(v, lo), hi);
}
__device__ __forceinline__ float rescale_rot(float x) {
#pragma clang fp contract(off)
  float v = x * 2.0f;
  v = v - 1.0f;
  return fminf(fmaxf(v, -1.0f), 1.0f);
}

}  // namespace

template <typename T>
__global__ __launch_bounds__(256) void act_sample_kernel(const ActSampleArgs p) {
  __shared__ int s_bin[kSeg];
  __shared__ float s_lp[kSeg], s_ent[kSeg];
  __shared__ float s_rank[4][kRankSlots];
  const ActSelectArgs& a = p.sel;
  const int r = blockIdx.x;            // output row
  const int rl = r / p.S;              // row of logits
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* __restrict__ row = a.logits + (long long)rl * 700;
  const float ninf = -__builtin_inff();
  const bool use_k = p.top_k > 0, use_p = p.top_p < 1.0f;
  float temp = 1.0f;
  if (p.temp) {
    temp = p.temp[rl];
    if (!(temp == temp)) temp = 1.0f;
    temp = fminf(fmaxf(temp, 1e-4f), 1e4f);
  }
  float* __restrict__ slots = s_rank[wave];

#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int d = wave * 3 + j;
    const int n = seg_bins(d);
    const float* __restrict__ x = row + seg_off(d);
    const bool ok0 = lane < n, ok1 = lane + 64 < n;
    float x0 = ok0 ? x[lane] : ninf;
    float x1 = ok1 ? x[lane + 64] : ninf;
    if (p.temp) {
      if (ok0) x0 = __fdiv_rn(x0, temp);
      if (ok1) x1 = __fdiv_rn(x1, temp);
    }
    const float m = wave_max(fmaxf(x0, x1));   // NaNs are ignored by fmaxf; the maximum has rank 0 and is in K under every filter
    int cand = (ok0 && x0 == m) ? lane : (ok1 && x1 == m) ? lane + 64 : 0x7fffffff;
    cand = wave_min_i(cand);
    const int mode = cand == 0x7fffffff ? 0 : cand;
    int bin = mode;
    float e0 = ok0 ? expf(x0 - m) : 0.f;
    float e1 = ok1 ? expf(x1 - m) : 0.f;
    bool k0 = ok0, k1 = ok1;                   // membership of K
    const bool filtered = (use_k && p.top_k < n) || use_p;   // uniform over the workgroup
    if (filtered) {
      int r0 = 0, r1 = 0;                      // ranks: always in [0, n)
      for (int i = 0; i < n; ++i) {
        const float zi = i < 64 ? __shfl(x0, i, 64) : __shfl(x1, i - 64, 64);
        r0 += (zi > x0 || (zi == x0 && i < lane)) ? 1 : 0;
        r1 += (zi > x1 || (zi == x1 && i < lane + 64)) ? 1 : 0;
      }
      if (use_k && p.top_k < n) {
        k0 = ok0 && r0 < p.top_k;
        k1 = ok1 && r1 < p.top_k;
        e0 = k0 ? e0 : 0.f;
        e1 = k1 ? e1 : 0.f;
      }
      if (use_p) {
        const float s1 = wave_sum(e0 + e1);
        slots[lane] = 0.f;
        slots[lane + 64] = 0.f;
        wave_lds_sync();
        if (ok0) slots[r0] = e0;               // NaN-free logits: distinct ranks, one writer per slot (a NaN takes rank 0 too: in bounds)
        if (ok1) slots[r1] = e1;
        wave_lds_sync();
        const float a0 = slots[lane], a1 = slots[lane + 64];
        const float c0 = wave_incl_scan(a0, lane);
        const float t0 = __shfl(c0, 63, 64);
        const float c1 = t0 + wave_incl_scan(a1, lane);
        const float u0 = __shfl_up(c0, 1, 64), u1 = __shfl_up(c1, 1, 64);
        wave_lds_sync();
        slots[lane] = lane ? u0 : 0.f;         // mass of the ranks below
        slots[lane + 64] = lane ? u1 : t0;
        wave_lds_sync();
        const float b0 = ok0 ? slots[r0] : 0.f, b1 = ok1 ? slots[r1] : 0.f;
        wave_lds_sync();                       // the next segment clears the slots
        k0 = k0 && b0 / s1 < p.top_p;
        k1 = k1 && b1 / s1 < p.top_p;
        e0 = k0 ? e0 : 0.f;
        e1 = k1 ? e1 : 0.f;
      }
    }
    const float s = wave_sum(e0 + e1);
    const float lse = m + logf(s);
    const float p0 = e0 / s, p1 = e1 / s;
    float pl = (k0 && p0 > 0.f) ? p0 * (x0 - lse) : 0.f;
    pl += (k1 && p1 > 0.f) ? p1 * (x1 - lse) : 0.f;
    const float ent = -wave_sum(pl);
    const unsigned long long kb0 = __ballot(k0), kb1 = __ballot(k1);
    if (p.given) {
      const int k = d < 2 ? 0 : d < 6 ? 1 : d < 8 ? 2 : 3;
      const long long* ik = k == 0 ? a.idx[0] : k == 1 ? a.idx[1] : k == 2 ? a.idx[2] : a.idx[3];
      const long long g = ik[(long long)r * key_dims(k) + (d - key_first(k))];
      bin = g < 0 ? 0 : g > n - 1 ? n - 1 : (int)g;
    } else if (a.u) {   // inverse CDF over pi in bin order: the number of bins whose inclusive cumulative probability is <= u
      float uu = a.u[(long long)r * kSeg + d];
      uu = fminf(fmaxf(uu, 0.f), 0x1.fffffep-1f);   // [0, 1); a NaN becomes 0
      const float c0 = wave_incl_scan(e0, lane);
      const float t0 = __shfl(c0, 63, 64);
      const float c1 = t0 + wave_incl_scan(e1, lane);
      const int cnt = __popcll(__ballot(ok0 && c0 / s <= uu)) + __popcll(__ballot(ok1 && c1 / s <= uu));
      bin = min(cnt, n - 1);
      if (filtered) {   // rounding at the upper end can land past the last bin of K: the last bin of K at or below
        int b = bin >= 64 ? top_bit_at_or_below(kb1, bin - 64) : -1;
        b = b >= 0 ? b + 64 : top_bit_at_or_below(kb0, min(bin, 63));
        bin = b >= 0 ? b : mode;
      }
    }
    const float xa = __shfl(x0, bin & 63, 64), xb = __shfl(x1, bin & 63, 64);
    float lp = (bin < 64 ? xa : xb) - lse;
    if (!(((bin < 64 ? kb0 : kb1) >> (bin & 63)) & 1ull) && filtered) lp = ninf;
    if (lane == 0) {
      s_bin[d] = bin;
      s_lp[d] = lp;
      s_ent[d] = ent;
    }
  }
  __syncthreads();

  const int t = threadIdx.x;
  if (t < kSeg) {   // the int64 bins in the layout vima_action_embed takes, and the continuous action
    const int k = t < 2 ? 0 : t < 6 ? 1 : t < 8 ? 2 : 3;
    const int i = t - key_first(k), w = key_dims(k);
    const int bin = s_bin[t];
    if (!p.given) {   // given bins are the caller's: left as they are
      long long* ik = k == 0 ? a.idx[0] : k == 1 ? a.idx[1] : k == 2 ? a.idx[2] : a.idx[3];
      ik[(long long)r * w + i] = bin;
    }
    if (a.cont) {
      float v = (float)bin / (float)seg_bins(t);
      if (a.has_bounds) v = (k & 1) ? rescale_rot(v) : rescale(v, i == 0 ? a.low[0] : a.low[1], i == 0 ? a.high[0] : a.high[1]);
      a.cont[(long long)r * kSeg + t] = v;
    }
  } else if (t >= 64 && t < 68) {   // per key: log-probability of the chosen bins and entropy, summed over the key's dimensions
    const int k = t - 64, f = key_first(k), w = key_dims(k);
    float lp = s_lp[f], en = s_ent[f];
    for (int i = 1; i < w; ++i) {
      lp += s_lp[f + i];
      en += s_ent[f + i];
    }
    if (a.logp) a.logp[(long long)r * 4 + k] = lp;
    if (a.ent) a.ent[(long long)r * 4 + k] = en;
  }

  if (a.t1) {   // first layer of the action embedding (action_embd.py:29-56), arithmetic of action_l1_kernel
    T* __restrict__ out = reinterpret_cast<T*>(a.t1) + (long long)r * 1024;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int K = key_dims(k), f = key_first(k);
      const float* __restrict__ W = a.w0[k] + t * K;
      float v = 0.f;
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const float bins = (K == 2 && i == 1) ? 100.0f : 50.0f;
        const float x = (float)s_bin[f + i] / bins;
        v = i == 0 ? x * W[0] : fmaf(x, W[i], v);
      }
      v += a.b0[k][t];
      Elem<T>::store(out + k * 256 + t, fmaxf(v, 0.f));
    }
  }
}

int launch_act_sample(const ActSampleArgs& p, bool is_bf16, hipStream_t st) {
  const ActSelectArgs& a = p.sel;
  if (a.R <= 0) return 0;
  if (!a.logits || !a.idx[0] || !a.idx[1] || !a.idx[2] || !a.idx[3] || p.S < 1 || !(p.top_p > 0.f)) return (int)hipErrorInvalidValue;
  if (a.t1) for (int k = 0; k < 4; ++k) if (!a.w0[k] || !a.b0[k]) return (int)hipErrorInvalidValue;
  if (is_bf16) hipLaunchKernelGGL(act_sample_kernel<bf16_t>, dim3(a.R), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(act_sample_kernel<float>, dim3(a.R), dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

}  // namespace vima
