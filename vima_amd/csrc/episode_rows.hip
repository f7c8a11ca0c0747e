// Episode caches, the per-sample plumbing both policy families share (XAttnGPT: vima_decode_*, decoder-only baselines: vima_seq_*): the ONE copy
// between a compact buffer of rows and the samples' blocks of a cache, the restart of listed samples and the install of a history's episode state.
//
// kv_rows_kernel moves n x L rows of N elements between a compact buffer (sample r = rows r L .., leading dimension ld) and a cache of Lc rows per
// sample: block list[r] (no list: r), row rowmap[l] (no map: l), the block row-major [Lc][N] or head-major [N / D][Lc][D] (the prompt K / V
// cache's two layouts), in either direction. It knows no operand type: the launcher counts N, ld and D of KvRowsArgs in 16-byte vectors, one
// uint4 load and one uint4 store per thread, a grid of (vectors of a sample, samples). What the callers do with it:
//   one sample's K | V rows into its head-major block (vima_decode_restart, the per-sample loop)                 n = 1, D
//   the K | V rows of the flagged samples into / out of the prompt K / V cache (batched restart / history)       list, D or 0, both directions
//   the k | v columns of a dense q | k | v into the episode cache (vima_seq_prefill, vima_seq_decode_restart)    ld = 3E, optional list, Lc > L
//   the same at the cache rows of a history (vima_decode_restart_history, vima_seq_decode_restart_history)       list and rowmap
// Plain loads and stores; list and rowmap entries are the caller's to keep inside the cache.
#include "kernels.h"

namespace vima {

// The fields of KvRowsArgs as plain kernel arguments (N, ld, D in 16-byte vectors; D = N for a row-major block: one piece per row). A launch of a
// few microseconds feels every dependent scalar load, so the body is straight-line code: no early exit (the index is clamped into the sample and
// only the store is predicated), layout and direction are selects. L * N < 2^31 (the launcher checks): 32-bit divisions.
__global__ __launch_bounds__(256) void kv_rows_kernel(const uint4* __restrict__ in, uint4* __restrict__ out, const int* __restrict__ list,
                                                      const int* __restrict__ rowmap, int L, int N, long long ld, int Lc, int D, int to_cache) {
  const int r = blockIdx.y;
  const unsigned i = blockIdx.x * 256u + threadIdx.x, total = (unsigned)(L * N);
  const unsigned k = i < total ? i : total - 1;
  const int l = (int)(k / (unsigned)N), c = (int)(k % (unsigned)N);
  const int b = list ? list[r] : r, row = rowmap ? rowmap[l] : l;
  const int piece = c / D;
  const long long compact = ((long long)r * L + l) * ld + c;
  const long long cache = (long long)b * Lc * N + ((long long)piece * Lc + row) * D + (c - piece * D);
  const uint4 v = to_cache ? in[compact] : in[cache];
  if (i < total) out[to_cache ? cache : compact] = v;
}

// Per-sample restart, one workgroup per listed sample b: the key-mask bytes of its rows [lo, hi) cleared (every cached key of the old episode
// masked), its next action slot marked absent (fresh[b] = 1, consumed by the next chunk's embedding) and, where the family counts positions from
// the episode's start (poscnt given), the counter back at 0.
__global__ __launch_bounds__(256) void episode_restart_kernel(const int* __restrict__ list, uint8_t* mask, int* poscnt, uint8_t* fresh, int lo,
                                                              int hi, int Lmax) {
  const int b = list[blockIdx.x];
  for (int i = lo + threadIdx.x; i < hi; i += 256) mask[(long long)b * Lmax + i] = 0;
  if (threadIdx.x == 0) {
    fresh[b] = 1;
    if (poscnt) poscnt[b] = 0;
  }
}

// The episode state of an installed history, one workgroup per listed sample b = list[r]: rows [lo, hi) masked (what episode_restart_kernel does;
// empty where the restart ran in front), then the key mask of the L compact rows of the call (mask [n, L]) at the cache rows rowmap[l] (DEVICE array
// [L], shared by the samples), poscnt[b] = the number of valid rows and fresh[b] = 0: the sample is mid-episode, its next step consumes its action
// token. The count is an integer <= Lmax: exact in the float reduction.
__global__ __launch_bounds__(256) void episode_install_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ list,
                                                              const int* __restrict__ rowmap, int L, int lo, int hi, int Lmax, uint8_t* cache_mask,
                                                              int* poscnt, uint8_t* fresh) {
  __shared__ float part[4];
  const int r = blockIdx.x, b = list[r];
  for (int i = lo + threadIdx.x; i < hi; i += 256) cache_mask[(long long)b * Lmax + i] = 0;
  __syncthreads();   // the mapped rows below lie inside [lo, hi): written after the clearing
  float cnt = 0.f;
  for (int l = threadIdx.x; l < L; l += 256) {
    const uint8_t mk = mask[(long long)r * L + l] ? 1 : 0;
    cache_mask[(long long)b * Lmax + rowmap[l]] = mk;
    cnt += (float)mk;
  }
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    poscnt[b] = (int)((part[0] + part[1]) + (part[2] + part[3]));
    fresh[b] = 0;
  }
}

int launch_kv_rows(const KvRowsArgs& a, int elem_bytes, hipStream_t st) {
  if (a.n <= 0 || a.L <= 0 || a.N <= 0) return 0;
  if (elem_bytes != 2 && elem_bytes != 4) return (int)hipErrorInvalidValue;
  const int epv = 16 / elem_bytes;   // elements per 16-byte vector
  if (a.N % epv || a.ld % epv || a.ld < a.N || a.D < 0 || (a.D > 0 && (a.D % epv || a.N % a.D)) || a.L > a.Lc || a.n > 65535 || !a.in || !a.out ||
      ((uintptr_t)a.in & 15) || ((uintptr_t)a.out & 15))
    return (int)hipErrorInvalidValue;
  const int N = a.N / epv;
  if ((long long)a.L * N >= (1ll << 31) - 256) return (int)hipErrorInvalidValue;   // the kernel's 32-bit vector index
  const dim3 grid((unsigned)(((long long)a.L * N + 255) / 256), (unsigned)a.n);
  hipLaunchKernelGGL(kv_rows_kernel, grid, dim3(256), 0, st, reinterpret_cast<const uint4*>(a.in), reinterpret_cast<uint4*>(a.out), a.list, a.rowmap,
                     a.L, N, a.ld / epv, a.Lc, a.D > 0 ? a.D / epv : N, a.to_cache ? 1 : 0);
  return (int)hipGetLastError();
}

int launch_episode_restart(const int* list, int n, uint8_t* mask, int* poscnt, uint8_t* fresh, int lo, int hi, int Lmax, hipStream_t st) {
  if (n <= 0) return 0;
  if (lo < 0 || hi > Lmax || !list || !mask || !fresh) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(episode_restart_kernel, dim3(n), dim3(256), 0, st, list, mask, poscnt, fresh, lo, hi, Lmax);
  return (int)hipGetLastError();
}

int launch_history_install(const uint8_t* mask, const int* list, const int* rowmap, int n, int L, int lo, int hi, int Lmax, uint8_t* cache_mask,
                           int* poscnt, uint8_t* fresh, hipStream_t st) {
  if (n <= 0) return 0;
  if (L <= 0 || L > Lmax || lo < 0 || hi > Lmax || !mask || !list || !rowmap || !cache_mask || !poscnt || !fresh) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(episode_install_kernel, dim3(n), dim3(256), 0, st, mask, list, rowmap, L, lo, hi, Lmax, cache_mask, poscnt, fresh);
  return (int)hipGetLastError();
}

}  // namespace vima
