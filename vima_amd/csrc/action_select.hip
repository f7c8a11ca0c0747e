// Action selection on the device: the step between the 700 raw logits of the action head and the next action token.
//
// Replaces, for the env-step loop, the host-side MultiCategorical wrapper (vima_amd/dists.py: 12 torch Categoricals, one logsumexp
// each, softmax + argmax per dimension), the de-discretisation / rescaling / clamping of the bins (vima_policy.py:301-322,
// scripts/example.py:213-234) and the first layer of the action embedding (action_l1_kernel, four launches that re-read the int64
// bins) by ONE launch: one 256-thread workgroup per row of logits.
//
// Phase 1: each of the four waves owns three of the twelve segments (kHeadBins: 50 100 | 50 50 50 50 | 50 100 | 50 50 50 50); a lane
//          holds at most two logits of a segment and everything is a wave reduction -- no atomics, no scratch.
// Phase 2: (only when the embedded token is asked for) after the one barrier thread n computes output n of the embedding's first
//          layer for the four keys from the bins in LDS, with the arithmetic of action_l1_kernel, so that the token is bit-identical
//          to vima_action_embed on the same bins.
#include "kernels.h"

namespace vima {

namespace {

constexpr int kSeg = 12;

__device__ __forceinline__ int seg_bins(int d) { return (d == 1 || d == 7) ? 100 : 50; }
__device__ __forceinline__ int seg_off(int d) { return 50 * d + (d > 1 ? 50 : 0) + (d > 7 ? 50 : 0); }
// key (pose0_position, pose0_rotation, pose1_position, pose1_rotation) of a dimension, its first dimension, its width
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

// bin / bins rescaled to the environment's bounds: every operation rounded to fp32 on its own (no fma contraction), which is what
// the torch expressions of the reference loop compute
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
__global__ __launch_bounds__(256) void act_select_kernel(const ActSelectArgs a) {
  __shared__ int s_bin[kSeg];
  __shared__ float s_lp[kSeg], s_ent[kSeg];
  const int r = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* __restrict__ row = a.logits + (long long)r * 700;
  const float ninf = -__builtin_inff();

#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int d = wave * 3 + j;
    const int n = seg_bins(d);
    const float* __restrict__ x = row + seg_off(d);
    const bool ok0 = lane < n, ok1 = lane + 64 < n;
    const float x0 = ok0 ? x[lane] : ninf;
    const float x1 = ok1 ? x[lane + 64] : ninf;
    const float m = wave_max(fmaxf(x0, x1));   // NaNs are ignored by fmaxf
    // first index of the maximum (exact comparison, torch.argmax); a row of NaNs has none and takes bin 0
    int cand = (ok0 && x0 == m) ? lane : (ok1 && x1 == m) ? lane + 64 : 0x7fffffff;
    cand = wave_min_i(cand);
    int bin = cand == 0x7fffffff ? 0 : cand;
    const float e0 = ok0 ? expf(x0 - m) : 0.f;
    const float e1 = ok1 ? expf(x1 - m) : 0.f;
    const float s = wave_sum(e0 + e1);
    const float lse = m + logf(s);
    // entropy = -sum p log p, log p = x - lse; a bin of probability 0 contributes 0
    const float p0 = e0 / s, p1 = e1 / s;
    float pl = (ok0 && p0 > 0.f) ? p0 * (x0 - lse) : 0.f;
    pl += (ok1 && p1 > 0.f) ? p1 * (x1 - lse) : 0.f;
    const float ent = -wave_sum(pl);
    if (a.u) {   // inverse CDF: the number of bins whose inclusive cumulative probability is <= u
      float uu = a.u[(long long)r * kSeg + d];
      uu = fminf(fmaxf(uu, 0.f), 0x1.fffffep-1f);   // [0, 1); a NaN becomes 0
      const float c0 = wave_incl_scan(e0, lane);
      const float t0 = __shfl(c0, 63, 64);
      const float c1 = t0 + wave_incl_scan(e1, lane);
      const int cnt = __popcll(__ballot(ok0 && c0 / s <= uu)) + __popcll(__ballot(ok1 && c1 / s <= uu));
      bin = min(cnt, n - 1);
    }
    const float xa = __shfl(x0, bin & 63, 64), xb = __shfl(x1, bin & 63, 64);
    const float lp = (bin < 64 ? xa : xb) - lse;
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
    long long* ik = k == 0 ? a.idx[0] : k == 1 ? a.idx[1] : k == 2 ? a.idx[2] : a.idx[3];   // selects: no indexing of the argument block by a lane value
    ik[(long long)r * w + i] = bin;
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

int launch_act_select(const ActSelectArgs& a, bool is_bf16, hipStream_t st) {
  if (a.R <= 0) return 0;
  if (!a.logits || !a.idx[0] || !a.idx[1] || !a.idx[2] || !a.idx[3]) return (int)hipErrorInvalidValue;
  if (a.t1) for (int k = 0; k < 4; ++k) if (!a.w0[k] || !a.b0[k]) return (int)hipErrorInvalidValue;
  if (is_bf16) hipLaunchKernelGGL(act_select_kernel<bf16_t>, dim3(a.R), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(act_select_kernel<float>, dim3(a.R), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace vima
