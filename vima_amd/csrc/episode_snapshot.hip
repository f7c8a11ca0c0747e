// Episode snapshots: a sample's episode state packed into a caller's payload and unpacked from it later, into any slot of any matching handle
// (vima_decode_snapshot / vima_decode_restore and the vima_seq_* pair; semantics and payload format in include/vima_hip.h, row bookkeeping in
// episode_book.h: steps_of / history_rows).
//
// episode_pack_kernel<T> / episode_unpack_kernel<T> keep the shape of episode_fork_kernel: one launch covers every layer and every listed sample of a
// cache [NL][B][L][N]; a grid-stride loop over flat work units on min(units, 2048) workgroups; a unit finds its job (SnapJob, kernels.h) by
// bisection over the jobs' unit prefix (uniform over the workgroup: scalar loads). Where fork moves contiguous spans, a snapshot moves ROWS: compact
// row k of a job lives at cache row map[map0 + k] -- the rows the last batch steps wrote, in time order, wherever the ring holds them -- so a unit
// is a chunk of rpc whole rows (about kSnapChunk 16-byte vectors) and every lane resolves the row of each of its four vectors from the table. The
// table is ONE per call: compact row k counted from the end is the same cache row whatever the episode's length, so every job reads a suffix.
// Four global_load_dwordx4 per lane are in flight together, unconditional at clamped (in-bounds) indices; only the stores are predicated. No LDS.
// The head-major prompt K / V layout ([N / D][L][D] per sample) is addressed as kv_rows_kernel (episode_rows.hip) does: a row's contiguous pieces
// are D elements; the payload is row-major [NL][rows][N] whatever the cache's layout.
// Plain loads and stores. Jobs of one unpack call name distinct samples, pack only reads the cache: no unit reads what another writes.
#include "kernels.h"

namespace vima {

template <typename T, bool PACK>
__device__ __forceinline__ void episode_snap_body(const EpisodeSnapArgs& a) {
  const int rv = (int)((long long)a.N * (long long)sizeof(T) / 16);   // 16-byte vectors per row
  const int dv = a.D > 0 ? (int)((long long)a.D * (long long)sizeof(T) / 16) : rv;   // per contiguous piece of a row
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
    const SnapJob* __restrict__ jp = a.jobs + lo;
    const int row0 = (r - jp->unit0) * a.rpc;                      // first compact row of the unit
    const int left = jp->nrows - row0;                             // rows of the job from this unit on: >= 1
    const int n = (left < a.rpc ? left : a.rpc) * rv;              // vectors of the unit
    const int m0 = jp->map0 + row0;
    uint4* __restrict__ pay = reinterpret_cast<uint4*>(jp->payload + (long long)layer * jp->layer_stride) + (long long)row0 * rv;
    uint4* __restrict__ blk = base + ((long long)layer * a.B + jp->sample) * sample_v;
    for (int v0 = (int)threadIdx.x; v0 < n + (int)threadIdx.x; v0 += kSnapChunk) {   // uniform trip count; one trip unless a row exceeds the chunk
      // vector k of the unit, clamped into it: compact row k / rv of the unit, 16-byte column k % rv -> its place in the sample's block
      auto place = [&](int k, int& c) -> long long {
        c = k < n ? k : n - 1;
        const int row = c / rv, col = c - row * rv;
        const int crow = a.map ? a.map[m0 + row] : m0 + row;
        const int piece = col / dv;
        return ((long long)piece * a.L + crow) * dv + (col - piece * dv);   // row-major: dv = rv, piece = 0
      };
      int c0, c1, c2, c3;
      const long long o0 = place(v0, c0), o1 = place(v0 + 256, c1), o2 = place(v0 + 512, c2), o3 = place(v0 + 768, c3);
      const bool p0 = v0 < n, p1 = v0 + 256 < n, p2 = v0 + 512 < n, p3 = v0 + 768 < n;
      // unconditional loads at clamped (in-bounds) indices: four loads in flight; only the stores are predicated
      if (PACK) {
        const uint4 x0 = blk[o0], x1 = blk[o1], x2 = blk[o2], x3 = blk[o3];
        if (p0) pay[c0] = x0;
        if (p1) pay[c1] = x1;
        if (p2) pay[c2] = x2;
        if (p3) pay[c3] = x3;
      } else {
        const uint4 x0 = pay[c0], x1 = pay[c1], x2 = pay[c2], x3 = pay[c3];
        if (p0) blk[o0] = x0;
        if (p1) blk[o1] = x1;
        if (p2) blk[o2] = x2;
        if (p3) blk[o3] = x3;
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void episode_pack_kernel(const EpisodeSnapArgs a) { episode_snap_body<T, true>(a); }

template <typename T>
__global__ __launch_bounds__(256) void episode_unpack_kernel(const EpisodeSnapArgs a) { episode_snap_body<T, false>(a); }

// one workgroup per (sample, payload) pair: the key-mask bytes of the episode's rows in compact order, the position counter and the fresh flag
__global__ __launch_bounds__(256) void episode_pack_state_kernel(const SnapStateJob* __restrict__ jobs, const int* __restrict__ map,
                                                                 const uint8_t* __restrict__ mask, const int* __restrict__ poscnt,
                                                                 const uint8_t* __restrict__ fresh, int Lmax) {
  const SnapStateJob j = jobs[blockIdx.x];
  const uint8_t* __restrict__ row = mask + (long long)j.sample * Lmax;
  uint8_t* __restrict__ out = reinterpret_cast<uint8_t*>(j.payload) + 16;
  for (int l = threadIdx.x; l < j.npre; l += 256) out[l] = row[l];
  for (int l = threadIdx.x; l < j.nrows; l += 256) out[j.npre + l] = row[map[j.map0 + l]];
  if (threadIdx.x == 0) *reinterpret_cast<int4*>(j.payload) = make_int4(poscnt[j.sample], (int)fresh[j.sample], j.nrows, 0);
}

// the restart of the slot (its mask row cleared over [lo, hi)), then the install: mask bytes to the mapped rows, counter and flag
__global__ __launch_bounds__(256) void episode_unpack_state_kernel(const SnapStateJob* __restrict__ jobs, const int* __restrict__ map, uint8_t* mask,
                                                                   int* __restrict__ poscnt, uint8_t* __restrict__ fresh, int Lmax, int lo, int hi) {
  const SnapStateJob j = jobs[blockIdx.x];
  uint8_t* row = mask + (long long)j.sample * Lmax;
  const uint8_t* __restrict__ in = reinterpret_cast<const uint8_t*>(j.payload) + 16;
  for (int l = lo + threadIdx.x; l < hi; l += 256) row[l] = 0;
  __syncthreads();   // the mapped rows lie inside [lo, hi): written after the clearing
  for (int l = threadIdx.x; l < j.npre; l += 256) row[l] = in[l];
  for (int l = threadIdx.x; l < j.nrows; l += 256) row[map[j.map0 + l]] = in[j.npre + l];
  if (threadIdx.x == 0) {
    const int4 hd = *reinterpret_cast<const int4*>(j.payload);
    poscnt[j.sample] = hd.x;
    fresh[j.sample] = (uint8_t)hd.y;
  }
}

static int snap_check(const EpisodeSnapArgs& a, bool is_bf16) {
  if (!a.cache || !a.jobs || a.NL <= 0 || a.B <= 0 || a.L <= 0 || a.N <= 0 || a.D < 0 || a.rpc <= 0) return (int)hipErrorInvalidValue;
  const long long es = is_bf16 ? 2 : 4;
  if ((a.N * es) % 16 || (reinterpret_cast<uintptr_t>(a.cache) & 15)) return 22;
  if (a.D > 0 && ((a.D * es) % 16 || a.N % a.D)) return 22;
  if (a.N * es / 16 >= (1ll << 24)) return (int)hipErrorInvalidValue;   // a unit's vector count stays far inside int
  if ((long long)a.NL * a.units >= (1ll << 31) - 2048) return (int)hipErrorInvalidValue;
  return 0;
}

int launch_episode_pack(const EpisodeSnapArgs& a, bool is_bf16, hipStream_t st) {
  if (a.n_jobs <= 0 || a.units <= 0) return 0;
  if (int e = snap_check(a, is_bf16)) return e;
  const long long total = (long long)a.NL * a.units;
  const unsigned grid = (unsigned)(total < 2048 ? total : 2048);
  if (is_bf16) hipLaunchKernelGGL(episode_pack_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(episode_pack_kernel<float>, dim3(grid), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

int launch_episode_unpack(const EpisodeSnapArgs& a, bool is_bf16, hipStream_t st) {
  if (a.n_jobs <= 0 || a.units <= 0) return 0;
  if (int e = snap_check(a, is_bf16)) return e;
  const long long total = (long long)a.NL * a.units;
  const unsigned grid = (unsigned)(total < 2048 ? total : 2048);
  if (is_bf16) hipLaunchKernelGGL(episode_unpack_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(episode_unpack_kernel<float>, dim3(grid), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

int launch_episode_pack_state(const SnapStateJob* jobs, int n, const int* map, const uint8_t* mask, const int* poscnt, const uint8_t* fresh, int Lmax,
                              hipStream_t st) {
  if (n <= 0) return 0;
  if (!jobs || !mask || !poscnt || !fresh || Lmax <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(episode_pack_state_kernel, dim3(n), dim3(256), 0, st, jobs, map, mask, poscnt, fresh, Lmax);
  return (int)hipGetLastError();
}

int launch_episode_unpack_state(const SnapStateJob* jobs, int n, const int* map, uint8_t* mask, int* poscnt, uint8_t* fresh, int Lmax, int lo, int hi,
                                hipStream_t st) {
  if (n <= 0) return 0;
  if (!jobs || !mask || !poscnt || !fresh || Lmax <= 0 || lo < 0 || hi > Lmax) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(episode_unpack_state_kernel, dim3(n), dim3(256), 0, st, jobs, map, mask, poscnt, fresh, Lmax, lo, hi);
  return (int)hipGetLastError();
}

}  // namespace vima
