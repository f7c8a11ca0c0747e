// Episode fork: a sample's episode state copied into other batch slots of the same caches, in place (vima_decode_fork / vima_seq_decode_fork;
// semantics in include/vima_hip.h, row bookkeeping in episode_book.h: fork_ok / live_ranges).
//
// episode_fork_kernel<T> moves row ranges of a per-sample cache [NL][B][L][N] of the operand type from source sample blocks to destination sample
// blocks. A range of a sample is one contiguous span per layer; a job (ForkJob, kernels.h) is one span and the destinations it goes to, cut into
// chunks of kForkChunk 16-byte vectors. A work unit = (layer, job, chunk): the workgroup loads the chunk ONCE -- four global_load_dwordx4 per
// lane, all in flight together -- and stores it to every destination of the job, so a source with d destinations moves 1 + d units of traffic
// and not 2 d. Plain loads and plain stores: the stores keep their lines in the XCD's L2, where the next env step's attention reads them; there
// is no hand-off inside the launch, so no other store flavour buys anything. The prompt K / V cache goes through the same kernel: a sample's
// block is contiguous in its row-major and in its head-major layout, one range of Lp rows of 2E either way.
// The grid is a grid-stride loop over the flat unit number, min(units, 2048) workgroups whatever B; a unit finds its job by bisection over the
// jobs' unit prefix (uniform over the workgroup: scalar loads).
// Sources and destinations are disjoint sets (EpisodeBook::fork_ok), so no unit reads what another writes.
#include "kernels.h"

namespace vima {

template <typename T>
__global__ __launch_bounds__(256) void episode_fork_kernel(const EpisodeForkArgs a) {
  const long long rv = (long long)a.N * (long long)sizeof(T) / 16;   // 16-byte vectors per row
  const long long sample_v = (long long)a.L * rv;
  uint4* __restrict__ base = reinterpret_cast<uint4*>(a.cache);
  const int total = a.NL * a.units;   // < 2^31: the launcher checks
  for (int u = blockIdx.x; u < total; u += gridDim.x) {
    const int layer = u / a.units, r = u - layer * a.units;
    int lo = 0, hi = a.n_jobs - 1;   // the last job whose unit0 <= r
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (a.jobs[mid].unit0 <= r) lo = mid;
      else hi = mid - 1;
    }
    const ForkJob* __restrict__ jp = a.jobs + lo;
    const int j_src = jp->src, j_dst0 = jp->dst0, j_ndst = jp->ndst, chunk = r - jp->unit0;
    const long long off = (long long)jp->row0 * rv + (long long)chunk * kForkChunk;   // in the sample's block
    const long long left = (long long)jp->nrows * rv - (long long)chunk * kForkChunk;   // vectors of the span from this chunk on: >= 1
    const int n = left < kForkChunk ? (int)left : kForkChunk;
    const uint4* __restrict__ s = base + ((long long)layer * a.B + j_src) * sample_v + off;
    const int k = (int)threadIdx.x;
    const bool p0 = k < n, p1 = k + 256 < n, p2 = k + 512 < n, p3 = k + 768 < n;
    // unconditional loads at clamped (in-bounds) indices: four loads in flight, no select between addresses; only the stores are predicated
    const uint4 v0 = s[min(k, n - 1)], v1 = s[min(k + 256, n - 1)], v2 = s[min(k + 512, n - 1)], v3 = s[min(k + 768, n - 1)];
    for (int d = 0; d < j_ndst; ++d) {
      uint4* __restrict__ o = base + ((long long)layer * a.B + a.dsts[j_dst0 + d]) * sample_v + off;
      if (p0) o[k] = v0;
      if (p1) o[k + 256] = v1;
      if (p2) o[k + 512] = v2;
      if (p3) o[k + 768] = v3;
    }
  }
}

// one workgroup per (destination, source) pair
__global__ __launch_bounds__(256) void episode_fork_state_kernel(const int* __restrict__ dsts, const int* __restrict__ srcs, uint8_t* __restrict__ mask,
                                                                 int* __restrict__ poscnt, uint8_t* __restrict__ fresh, int Lmax) {
  const int d = dsts[blockIdx.x], s = srcs[blockIdx.x];
  for (int l = threadIdx.x; l < Lmax; l += 256) mask[(long long)d * Lmax + l] = mask[(long long)s * Lmax + l];
  if (threadIdx.x == 0) {
    poscnt[d] = poscnt[s];
    fresh[d] = fresh[s];
  }
}

int launch_episode_fork(const EpisodeForkArgs& a, bool is_bf16, hipStream_t st) {
  if (a.n_jobs <= 0 || a.units <= 0) return 0;
  if (!a.cache || !a.jobs || !a.dsts || a.NL <= 0 || a.B <= 0 || a.L <= 0 || a.N <= 0) return (int)hipErrorInvalidValue;
  if (((long long)a.N * (is_bf16 ? 2 : 4)) % 16 || (reinterpret_cast<uintptr_t>(a.cache) & 15)) return 22;
  const long long total = (long long)a.NL * a.units;
  if (total >= (1ll << 31) - 2048) return (int)hipErrorInvalidValue;
  const unsigned grid = (unsigned)(total < 2048 ? total : 2048);
  if (is_bf16) hipLaunchKernelGGL(episode_fork_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(episode_fork_kernel<float>, dim3(grid), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

int launch_episode_fork_state(const int* dsts, const int* srcs, int n, uint8_t* mask, int* poscnt, uint8_t* fresh, int Lmax, hipStream_t st) {
  if (n <= 0) return 0;
  if (!dsts || !srcs || !mask || !poscnt || !fresh || Lmax <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(episode_fork_state_kernel, dim3(n), dim3(256), 0, st, dsts, srcs, mask, poscnt, fresh, Lmax);
  return (int)hipGetLastError();
}

}  // namespace vima
