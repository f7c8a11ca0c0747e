// gemm_q4_kernel: 256 x 384 persistent bf16 GEMM with FOUR waves -- one per SIMD, the whole 512-entry register file each (round 6).
// Included by gemm.hip inside namespace vima { namespace { (after tile_epilogue_256, whose arithmetic it shares).
//
// Why it was built: the 256x256 ping-pong kernel (gemm_pp_kernel) moves 64 KiB of operands per 8.4 MFLOP K-tile through the L2 -> CU path, a 256x384 tile 80 KiB
// per 12.6 MFLOP (-17 % bytes per FLOP), and rounds 1-5 read that path as the bound. What it showed (DESIGN.md 4.2c, 4.6): 91.7 % of the matrix pipe in the K-loop,
// 7 % fewer busy cycles per launch than the 8-wave kernel -- and the same wall time, because these GEMMs run at the clock the chip's power budget grants them.
// Opt-in (gemm_q4). Its 384 accumulator registers per wave (128 x 192 outputs) do not fit two waves per SIMD, so there is no partner wave to overlap with: ONE
// instruction stream per SIMD carries the MFMAs with everything else (fragment reads, LDS-DMA requests, the counted wait, the barrier) placed between them.
//
// Schedule. A K-tile (64 k) is four LDS slots: A0 / A1 (tile rows [64h, 64h+64) of both wave rows: 128 x 128 B = 16 KiB) and B0 / B1 (W rows
// [96h, 96h+96) of both wave columns: 192 x 128 B = 24 KiB); two stages of 80 KiB fill the LDS. A wave (wm, wn) walks the four quadrants of its
// 128 x 192 block in Gray-code order, one operand set changing per step:
//      P1 (A0,B0)   P2 (A1,B0)   P3 (A1,B1)   P4 (A0,B1)   | next K-tile: P1 (A0',B0') ...
// 24 MFMAs (2 mi x 3 ni x 4 k-steps = 768 matrix-pipe clocks) per phase. The fragments of the operand that changes are re-loaded IN PLACE, k-step by
// k-step, as the current phase retires them ("rolling": after the MFMAs of k-step kk, registers [kk] receive the next phase's values), so a fragment
// read has a whole phase to arrive and only 80 fragment registers are live. Slots are recycled as soon as the protocol allows:
//      P1(t) requests A0(t+1)   P2(t) B0(t+2)   P3(t) A1(t+2)   P4(t) B1(t+2)          (t = K-tile of the stream; stage = t & 1)
//   WAR: a slot last READ during phase p is requested again in phase p + 2 at the earliest -- the reads issued in p are consumed by MFMAs of p + 1,
//        i.e. complete in every wave before the barrier that ends p + 1; no lgkmcnt wait is ever exposed for it;
//   RAW: one counted wait per K-tile, `s_waitcnt vmcnt(10)` before the barrier that ends P3(t): it retires A0(t+1) (requested in P1(t); the 6 + 4
//        pieces of P2 / P3 stay in flight), and everything older; P4(t) then starts reading A0(t+1) / B0(t+1). VMEM loads retire in order.
// One barrier per phase (four waves, no ping-pong partner). A0 is read twice per K-tile (P4 of the previous tile and P3), which is why its request
// comes last and has the shortest lead (3 phases); the other slots are requested 6 phases before their first read.
// Output tiles: the K-tiles of all tiles of a workgroup form one stream (requests run into the next tile's K-tiles 0 / 1 during the last two
// K-tiles); at the end of a tile slot A0 of stage 1 is free (nk is even) and holds the four 4-KiB epilogue slabs; the last phase of a tile does its
// rolling reads like every other (ONE loop body: see the note at the loop) but nobody uses them: the fragments would have to live through the epilogue,
// so the next tile starts with 20 cold fragment reads.
// Same MFMA (32x32x16 bf16, W fragment as the A operand), same K order as every other tile shape -> bit-identical results; the epilogue IS
// tile_epilogue_256_impl (NI = 6).
// Registers: 384 accumulators = 256 AGPRs + 128 VGPRs, 80 fragment VGPRs, 16 LDS address VGPRs. hipcc cannot be left to allocate this: (1) it gives
// every builtin MFMA of an AGPR-using kernel an AGPR destination and shuttles the 128 accumulators that do not fit through v_accvgpr moves around
// every MFMA; (2) it spreads the in-place fragment reloads over 108 registers and spills addresses into the loop (each reload = `s_waitcnt vmcnt(0)`
// = the LDS-DMA stream drained). So the MFMAs and the fragment reads are inline asm with tied operands -- the accumulator's register FILE is chosen
// per accumulator ("+a" / "+v"), a fragment keeps ONE register tuple for the whole kernel ("+v") -- and the lgkmcnt waits in front of the MFMAs are
// counted by hand (LDS reads return in order; the main loop holds no scalar loads, tests/test_kernel_resources.py checks the ISA for that).
// MIH = 32-row blocks per wave and A half: 2 -> the 256 x 384 tile described above; 1 -> a 128 x 384 tile (wave tile 64 x 192, 12 MFMAs per phase, A slots of 8 KiB,
// epilogue slabs behind the ring) for problems whose 256-row tilings leave CUs idle: M = 16 384, N = 768 is 192 tiles of 256 x 256 but 256 of 128 x 384.
// EPI 7 (256 x 384 only) = the bf16-output epilogue (1) of a fused-RMSNorm CONSUMER without bias: every accumulator row is multiplied by
// rsqrt(sum of the row's 24 partials * rs_invk + rs_eps). The tile has no LDS left for the partials (the 128 x 384 tile parks them behind its ring) and the
// K loop no registers for them, so a lane carries the four finished scales of its rows through the K loop and the partials of the NEXT tile are fetched
// across the epilogue, when the 80 fragment registers are dead: see "row scales" in the kernel.
template <int MIH_>
struct Q4T {
  static constexpr int MIH = MIH_, RH = MIH_ * 32;             // rows of one A half per wave row
  static constexpr int BM = 4 * RH, BN = 384, MI = 2 * MIH_, NI = 6, NIH = 3, THREADS = 256;
  static constexpr int A_SLOT = 2 * RH * 128, B_SLOT = 24576;  // 16 / 8 KiB, 24 KiB
  static constexpr int PA = A_SLOT / 4096;                     // 1-KiB LDS-DMA pieces per wave and A slot (B slots: 6)
  static constexpr int OA0 = 0, OA1 = A_SLOT, OB0 = 2 * A_SLOT, OB1 = 2 * A_SLOT + B_SLOT;
  static constexpr int STAGE = 2 * A_SLOT + 2 * B_SLOT;        // 80 / 64 KiB
  static constexpr int SLAB_OFF = MIH_ == 2 ? STAGE + OA0 : 2 * STAGE;   // epilogue slabs (4 x 4 KiB): slot A0 of stage 1 | behind the ring
  static constexpr int RS_OFF = 2 * STAGE + 16384;            // 128 x 384 only: the tile's fused-RMSNorm partials (128 rows x 24 floats = 12 KiB) behind the slabs
  static constexpr int SMEM_BYTES = MIH_ == 2 ? 2 * STAGE : 2 * STAGE + 16384 + 128 * 96;   // 160 / 156 KiB
};
using Q4 = Q4T<2>;
template <int V> using QI = std::integral_constant<int, V>;
typedef unsigned q4_u32x4 __attribute__((ext_vector_type(4)));

// 16 of the 24 32x32 accumulator blocks live in AGPRs, the blocks ni % 3 == 2 in VGPRs. What the compiler no longer sees: the MFMA's result latency --
// the same accumulator is used again 6 MFMAs (>= 192 clocks) later, and every accumulator passes through the wait states of the asm statement behind the K loop before the epilogue reads it.
template <bool IN_VGPR>
__device__ __forceinline__ void q4_mma(f32x16_t& c, const q4_u32x4& w, const q4_u32x4& a) {
  if constexpr (IN_VGPR) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(w), "v"(a));
  else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(w), "v"(a));
}
// fragment read INTO THE REGISTERS f ALREADY HAS (the asm reads and writes f); completion is waited for with q4_lgkm
template <int OFF>
__device__ __forceinline__ void q4_lds(q4_u32x4& f, unsigned addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds_read offset field");
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "+v"(f) : "v"(addr), "n"(OFF));
}
template <int OFF>
__device__ __forceinline__ void q4_lds_new(q4_u32x4& f, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(f) : "v"(addr), "n"(OFF));
}
template <int N> __device__ __forceinline__ void q4_lgkm() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N)); }
// LDS-DMA piece without the M0 save / restore of glds16_asm_s: nothing else in this kernel uses M0 (checked in the ISA by tests/test_kernel_resources.py)
__device__ __forceinline__ void q4_glds(const void* sbase, unsigned voff, unsigned lds_byte_addr) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(sbase), "s"(lds_byte_addr) : "memory");
}

// one 16-byte global load into accumulator registers whose completion is OURS to wait for. hipcc knows neither the request nor WHEN the registers are
// written: to it the "=a" output is defined at this statement, so a register-allocator copy or reuse of these AGPRs between the request and rs_landed
// would read or clobber data that has not arrived. Nothing in the source can forbid that; it holds because the allocator has no other use for AGPRs
// there, and it was read off the listing (profiles/q4_rms_consumers_isa_digests.txt) -- RE-READ THE LISTING WHEN THE COMPILER CHANGES: only the
// bit-equality tests (tests/test_q4_rms_consumer_gpu.py, the headline q4 test of tests/test_policy_gpu.py) would catch it otherwise.
template <int OFF>
__device__ __forceinline__ void q4_gld(q4_u32x4& d, const void* sbase, unsigned voff) {
  asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=a"(d) : "v"(voff), "s"(sbase), "n"(OFF) : "memory");
}

template <int ACT, int EPI, int MIH = 2>
__global__ __launch_bounds__(Q4::THREADS) __attribute__((amdgpu_waves_per_eu(1, 1))) void gemm_q4_kernel(const GemmDev p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using QC = Q4T<MIH>;
  constexpr int MI = QC::MI, NI = QC::NI, STAGE = QC::STAGE, RH = QC::RH, PA = QC::PA;
  constexpr int OA0 = QC::OA0, OA1 = QC::OA1, OB0 = QC::OB0, OB1 = QC::OB1;
  constexpr bool RSQ = EPI == 7;                      // row scales held in registers (launcher: rs_ssq set, rs_parts == 24, no bias)
  constexpr int EPX = RSQ ? 1 : EPI;                  // the epilogue proper
  static_assert(!RSQ || MIH == 2, "the 128 x 384 tile keeps its partials in LDS (EPI 1 / 5)");
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  const int wm = w >> 1, wn = w & 1;
  const int G = gridDim.x;
  const int nk = p.K / 64;              // even, >= 2 (launcher)
  const char* A = reinterpret_cast<const char*>(p.A);
  const char* W = reinterpret_cast<const char*>(p.W);
  const unsigned ldaB = (unsigned)p.lda * 2u, ldwB = (unsigned)p.ldw * 2u;

  auto tile_at = [&](int v, int& tm, int& tn) {      // gemm_pp_kernel's raster: XCD v & 7 walks its A panels through groups of `ngroup` W panels
    const int idx = v >> 3;
    const int mtx = (p.mtiles + 7) >> 3;
    const int per_group = mtx * p.ngroup;
    const int g = idx / per_group;
    const int rem = idx - g * per_group;
    const int ng = min(p.ngroup, p.ntiles - g * p.ngroup);
    const int q = rem / ng;
    tn = g * p.ngroup + (rem - q * ng);
    tm = q * 8 + (v & 7);
  };
  auto next_valid = [&](int v) {
    while (v < p.vtotal) {
      int tm, tn;
      tile_at(v, tm, tn);
      if (tm < p.mtiles) return v;
      v += G;
    }
    return -1;
  };

  const unsigned smem_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  // fragment read addresses (LDS byte addresses): per stage and k-step one register for the A slots (slot A0 of the stage + this lane's row and swizzled
  // 16-B chunk; + 16384 for A1, + mi * 4096 as the instruction's offset) and one for the B slots (slot B0; + 24576 for B1, + ni * 4096)
  unsigned adA[2][4], adB[2][4];
  {
    const int sw = (l31 >> 1) & 7;
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const unsigned ch = (unsigned)(((kk * 2 + hi) ^ sw) << 4);
        adA[st][kk] = smem_base + (unsigned)(st * STAGE + OA0 + (wm * RH + l31) * 128) + ch;
        adB[st][kk] = smem_base + (unsigned)(st * STAGE + OB0 + (wn * 96 + l31) * 128) + ch;
      }
  }
  // LDS-DMA: piece i of a slot = slot rows [(4 i + w) * 8, + 8); lane -> row rl = 8 w + lane / 8 of the 32-row group, 16-B position lane & 7, global
  // chunk position ^ swz(row). Per lane ONE byte offset per operand; the piece's tile row and the K-tile are wave-uniform (scalar) offsets.
  const int rl = w * 8 + (lane >> 3);
  const unsigned chD = (unsigned)(((lane & 7) ^ ((rl >> 1) & 7)) << 4);
  const unsigned voffA = (unsigned)rl * ldaB + chD, voffW = (unsigned)rl * ldwB + chD;

  // ---- stream cursor: current and next output tile of this workgroup (byte offsets of their first A / W rows)
  int cv = next_valid(blockIdx.x);
  if (cv < 0) return;
  int nv = next_valid(cv + G);
  unsigned aC, wC, aN = 0, wN = 0;
  auto tile_offs = [&](int v, unsigned& a, unsigned& ww) {
    int tm, tn;
    tile_at(v, tm, tn);
    a = (unsigned)(tm * QC::BM) * ldaB;
    ww = (unsigned)(tn * QC::BN) * ldwB;
  };
  tile_offs(cv, aC, wC);
  if (nv >= 0) tile_offs(nv, aN, wN);
  // K-tile kq in the current output tile's numbering (kq >= nk: K-tile kq - nk of the NEXT tile) -> byte offsets of its first A / W row. Past the end
  // of the stream (no next tile) the request is still ISSUED -- for K-tile 0 of the current tile, into a slot nobody reads any more -- so that the
  // phases are branch-free and the wait count of P3 is a constant; the kernel ends with `s_waitcnt vmcnt(0)`.
  auto cursor = [&](int kq, unsigned& ra, unsigned& rw) {
    const bool cur = kq < nk, nxt = nv >= 0;
    const unsigned ko = (unsigned)(cur ? kq : (nxt ? kq - nk : 0)) * 128u;
    ra = (unsigned)__builtin_amdgcn_readfirstlane((int)(((cur || !nxt) ? aC : aN) + ko));   // (uniform by construction; keeps the address arithmetic on the scalar unit)
    rw = (unsigned)__builtin_amdgcn_readfirstlane((int)(((cur || !nxt) ? wC : wN) + ko));
  };
  auto pieceA = [&](int stq, int h, int i, unsigned ra) {   // stq, h, i: compile-time after unrolling
    const unsigned row = (unsigned)((i * 32 / RH) * (2 * RH) + h * RH + (i * 32) % RH);   // slot rows [32 i, 32 i + 32): wave row (32 i) / RH, its rows (32 i) % RH ..
    q4_glds(A + (ra + row * ldaB), voffA, smem_base + (unsigned)(stq * STAGE + (h ? OA1 : OA0) + (i * 4 + w) * 1024));
  };
  auto pieceB = [&](int stq, int h, int i, unsigned rw) {
    const unsigned row = (unsigned)((i / 3) * 192 + h * 96 + (i % 3) * 32);
    q4_glds(W + (rw + row * ldwB), voffW, smem_base + (unsigned)(stq * STAGE + (h ? OB1 : OB0) + (i * 4 + w) * 1024));
  };

  // ---- row scales (EPI 7). In the epilogue a lane needs the scales of rows wm * 128 + mi * 32 + l31, mi = 0 .. 3; lanes l31 and l31 + 32 need the same
  // four, so each of them fetches and sums TWO rows -- mi = 2 hi and 2 hi + 1: 2 x 24 floats = twelve 16-byte loads -- and one v_permlane32_swap per
  // value hands both halves all four. The loads are inline asm (hipcc would drain the LDS-DMA stream for a load it tracks) INTO ACCUMULATOR
  // REGISTERS: in VGPRs the allocator copied and spilled the 48 in-flight registers around the epilogue's own; AGPRs it has no other use for, and
  // the accumulators of a 32-row block are dead once the block is stored. The requests for the NEXT tile (behind a workgroup's last tile: the
  // current tile's rows again -- in bounds, never read: the loop leaves before rs_landed and the kernel's final vmcnt(0) covers them; they only keep
  // the epilogue branch-free) are issued in front of the epilogue's second 32-row block and waited for behind the epilogue and the cursor
  // arithmetic, with `vmcnt(0)`: a counted wait may only count younger LOADS (see tile_epilogue_256_impl), and what vmcnt(0) waits for besides are
  // the epilogue's stores and K-tile 1 of the next tile, requested a whole K-tile before the epilogue. The first tile's are requested between
  // K-tiles 0 and 1 of the prologue, whose own counted wait covers them. rsc holds the current tile's four scales through the K loop.
  float rsc[4] = {1.0f, 1.0f, 1.0f, 1.0f};
  auto rs_request = [&](int v, q4_u32x4 (&rq)[12]) {
    int tm, tn;
    tile_at(v, tm, tn);
    const unsigned off = (unsigned)(tm * QC::BM + wm * 128 + hi * 64 + l31) * 96u;   // (launcher: M * 96 < 2^32)
    q4_gld<0>(rq[0], p.rs_ssq, off); q4_gld<16>(rq[1], p.rs_ssq, off); q4_gld<32>(rq[2], p.rs_ssq, off);
    q4_gld<48>(rq[3], p.rs_ssq, off); q4_gld<64>(rq[4], p.rs_ssq, off); q4_gld<80>(rq[5], p.rs_ssq, off);
    q4_gld<3072>(rq[6], p.rs_ssq, off); q4_gld<3088>(rq[7], p.rs_ssq, off); q4_gld<3104>(rq[8], p.rs_ssq, off);
    q4_gld<3120>(rq[9], p.rs_ssq, off); q4_gld<3136>(rq[10], p.rs_ssq, off); q4_gld<3152>(rq[11], p.rs_ssq, off);
  };
  // every request passes through this statement before its registers are named again; DRAIN: with the wait (the prologue has its own)
  auto rs_landed = [&](auto drain_, q4_u32x4 (&rq)[12]) {
    if constexpr (decltype(drain_)::value)
      asm volatile("s_waitcnt vmcnt(0)" : "+a"(rq[0]), "+a"(rq[1]), "+a"(rq[2]), "+a"(rq[3]), "+a"(rq[4]), "+a"(rq[5]), "+a"(rq[6]), "+a"(rq[7]),
                   "+a"(rq[8]), "+a"(rq[9]), "+a"(rq[10]), "+a"(rq[11]) : : "memory");
    else
      asm volatile("" : "+a"(rq[0]), "+a"(rq[1]), "+a"(rq[2]), "+a"(rq[3]), "+a"(rq[4]), "+a"(rq[5]), "+a"(rq[6]), "+a"(rq[7]), "+a"(rq[8]),
                   "+a"(rq[9]), "+a"(rq[10]), "+a"(rq[11]) : : "memory");
    // ln_tree24's order, then rms_row_scale's arithmetic -> the same bits as every other tile shape
    auto f4 = [](const q4_u32x4& u) { return make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w)); };
    const float s0 = __builtin_amdgcn_rsqf(ln_tree24_v(f4(rq[0]), f4(rq[1]), f4(rq[2]), f4(rq[3]), f4(rq[4]), f4(rq[5])) * p.rs_invk + p.rs_eps);
    const float s1 = __builtin_amdgcn_rsqf(ln_tree24_v(f4(rq[6]), f4(rq[7]), f4(rq[8]), f4(rq[9]), f4(rq[10]), f4(rq[11])) * p.rs_invk + p.rs_eps);
    // swap(x, x): first result = the lower half's value in both halves (rows mi 0 / 1), second = the upper half's (rows mi 2 / 3)
    const auto x0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(s0), __float_as_uint(s0), false, false);
    const auto x1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(s1), __float_as_uint(s1), false, false);
    rsc[0] = __uint_as_float(x0[0]); rsc[1] = __uint_as_float(x1[0]); rsc[2] = __uint_as_float(x0[1]); rsc[3] = __uint_as_float(x1[1]);
  };

  // ---- prologue of the stream (K-tiles 0 and 1 of the first tile, nk >= 2), in the order the steady state would have requested them
  {
    q4_u32x4 rq[12];
    unsigned ra0, rw0, ra1, rw1;
    cursor(0, ra0, rw0);
    cursor(1, ra1, rw1);
#pragma unroll
    for (int i = 0; i < 6; ++i) pieceB(0, 0, i, rw0);
#pragma unroll
    for (int i = 0; i < PA; ++i) pieceA(0, 1, i, ra0);
#pragma unroll
    for (int i = 0; i < 6; ++i) pieceB(0, 1, i, rw0);
#pragma unroll
    for (int i = 0; i < PA; ++i) pieceA(0, 0, i, ra0);
    if constexpr (RSQ) rs_request(cv, rq);   // older than K-tile 1's 12 + PA pieces: retired by the wait below
#pragma unroll
    for (int i = 0; i < 6; ++i) pieceB(1, 0, i, rw1);
#pragma unroll
    for (int i = 0; i < PA; ++i) pieceA(1, 1, i, ra1);
#pragma unroll
    for (int i = 0; i < 6; ++i) pieceB(1, 1, i, rw1);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(12 + PA) : "memory");     // K-tile 0 has landed (the 6 + PA + 6 pieces of K-tile 1's B0 / A1 / B1 may be in flight)
    if constexpr (RSQ) rs_landed(QI<0>{}, rq);
  }

  q4_u32x4 fa[MIH][4], fb[3][4];

  while (true) {
    int tm, tn;
    tile_at(cv, tm, tn);
    const int m0 = tm * QC::BM, n0 = tn * QC::BN;
    auto stamp = [&](int slot) {
      if (p.dbg && tid == 0) {
        long long* d = p.dbg + (long long)cv * 8;
        d[slot] = (long long)__builtin_readcyclecounter();
        if (slot == 0) {
          d[4] = (long long)__builtin_amdgcn_s_memrealtime();
          d[6] = (long long)__builtin_amdgcn_s_getreg((31 << 11) | 4);
          d[7] = (long long)__builtin_amdgcn_s_getreg((31 << 11) | 20);
        }
        if (slot == 3) d[5] = (long long)__builtin_amdgcn_s_memrealtime();
      }
    };
    stamp(0);
    f32x16_t acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.0f;
    // K-tile 0 of this tile has landed in every wave (first tile: the prologue's wait; later: the wait of the previous tile's last P3) and every
    // wave is done with the epilogue slabs
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // Fused-RMSNorm consumer on the 128 x 384 tile (the 256 x 384 tile has no LDS left and carries its row scales in registers: EPI 7): wave w requests the partials of tile rows [32 w, 32 w + 32) -- 24 floats per
    // row, 3 KiB, contiguous -- by LDS-DMA into their own region. The requests are OLDER than every K-tile request this tile will issue, so the counted
    // waits of its P3 phases (at least two: nk >= 2) retire them and the phase barriers publish them; they are reduced after the loop, from LDS.
    const bool rs_on = MIH == 1 && (EPI == 1 || EPI == 5) && p.rs_ssq != nullptr;    // (launcher: rs_parts == 24)
    if constexpr (MIH == 1) {
      if (rs_on) {
        const char* src = reinterpret_cast<const char*>(p.rs_ssq) + (size_t)(m0 + w * 32) * 96;
        const unsigned dst = smem_base + (unsigned)(QC::RS_OFF + w * 3072);
        q4_glds(src, (unsigned)lane * 16u, dst);
        q4_glds(src + 1024, (unsigned)lane * 16u, dst + 1024);
        q4_glds(src + 2048, (unsigned)lane * 16u, dst + 2048);
      }
    }
    // first fragments (A0, B0 of stage 0), k-step by k-step in the order a P4 issues its rolling reads: P1's wait counts are the steady state's
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      q4_lds_new<0>(fa[0][kk], adA[0][kk]);
      q4_lds_new<0>(fb[0][kk], adB[0][kk]);
      q4_lds_new<4096>(fb[1][kk], adB[0][kk]);
      q4_lds_new<8192>(fb[2][kk], adB[0][kk]);
      if constexpr (MIH == 2) q4_lds_new<4096>(fa[MIH - 1][kk], adA[0][kk]);
    }
    stamp(1);

    // one phase: quadrant (A half AH, B half BH) x K = 64 of K-tile ktc (stage ST), with the rolling reload for the next phase (NX: 0 the A half
    // changes, 1 the B half changes, 2 both = the next K-tile's A0 / B0 in the other stage)
    auto phase = [&](auto st_, auto p_, auto nx_, int ktc) {
      constexpr int ST = decltype(st_)::value, P = decltype(p_)::value, NX = decltype(nx_)::value;
      constexpr int AH = (P == 2 || P == 3) ? 1 : 0, BH = P >= 3 ? 1 : 0;
      constexpr int NST = NX == 2 ? (ST ^ 1) : ST;                      // stage the rolling reads come from
      constexpr int NAO = NX == 2 ? 0 : (AH ? 0 : QC::A_SLOT);          // ... their A slot (A0: + 0, A1: + A_SLOT) ...
      constexpr int NBO = NX == 2 ? 0 : 24576;                          // ... and B slot (B0: + 0, B1: + 24576) relative to adA / adB of that stage
      // fragment reads issued per k-step by this phase and by the one before it (P1 <- P4 <- P3 <- P2 <- P1): the counted waits below
      constexpr int R_OWN = NX == 0 ? MIH : (NX == 1 ? 3 : 3 + MIH);
      constexpr int R_PREV = P == 1 ? 3 + MIH : (P == 2 ? MIH : (P == 3 ? 3 : MIH));
      unsigned ra, rw;
      cursor(ktc + (P == 1 ? 1 : 2), ra, rw);   // this phase's request: P1 A0(t+1) | P2 B0(t+2) | P3 A1(t+2) | P4 B1(t+2)
      __builtin_amdgcn_sched_barrier(0);
      auto kstep = [&](auto kk_) {
        constexpr int kk = decltype(kk_)::value;
        auto m = [&](auto mi_, auto ni_) {
          constexpr int mi = decltype(mi_)::value, ni = decltype(ni_)::value;
          q4_mma<(ni == 2)>(acc[AH * MIH + mi][BH * 3 + ni], fb[ni][kk], fa[mi][kk]);
        };
        auto dma = [&]() {   // the request pieces of this k-step: A slots 4 pieces (one per k-step), B slots 6 (2, 2, 1, 1)
          if constexpr (P == 1) { if (kk < PA) pieceA(ST ^ 1, 0, kk, ra); }
          if constexpr (P == 3) { if (kk < PA) pieceA(ST, 1, kk, ra); }
          if constexpr (P == 2 || P == 4) {
            constexpr int h = P == 2 ? 0 : 1;
            if (kk == 0) { pieceB(ST, h, 0, rw); pieceB(ST, h, 1, rw); }
            if (kk == 1) { pieceB(ST, h, 2, rw); pieceB(ST, h, 3, rw); }
            if (kk == 2) pieceB(ST, h, 4, rw);
            if (kk == 3) pieceB(ST, h, 5, rw);
          }
        };
        auto rA = [&](auto mi_) {   // rolling read of A fragment mi of the next phase into the registers k-step kk has just retired
          constexpr int mi = decltype(mi_)::value;
          q4_lds<NAO + mi * 4096>(fa[mi][kk], adA[NST][kk]);
        };
        auto rB = [&](auto ni_) {
          constexpr int ni = decltype(ni_)::value;
          q4_lds<NBO + ni * 4096>(fb[ni][kk], adB[NST][kk]);
        };
        constexpr QI<0> I0{}; constexpr QI<1> I1{}; constexpr QI<2> I2{};
        // the fragments of k-step kk were read at the latest during the previous phase's k-step kk; issued since: its k-steps kk + 1 .. 3 and this
        // phase's k-steps 0 .. kk - 1 (LDS reads return in order; lgkmcnt is a 4-bit counter: 15 is the largest count)
        q4_lgkm<(3 - kk) * R_PREV + kk * R_OWN>();
        if constexpr (MIH == 1) {         // 64 x 192 per wave: three MFMAs per k-step; a fragment retires with its MFMA
          m(I0, I0);
          dma();
          if constexpr (NX != 0) rB(I0);
          m(I0, I1);
          if constexpr (NX != 0) rB(I1);
          m(I0, I2);
          if constexpr (NX != 0) rB(I2);
          if constexpr (NX != 1) rA(I0);
        } else if constexpr (NX == 1) {   // ni-major: a B fragment retires after its two MFMAs
          m(I0, I0);
          dma();
          m(I1, I0);
          rB(I0);
          m(I0, I1); m(I1, I1);
          rB(I1);
          m(I0, I2); m(I1, I2);
          rB(I2);
        } else {                          // mi-major: A fragment 0 retires after three MFMAs
          m(I0, I0);
          dma();
          m(I0, I1); m(I0, I2);
          rA(I0);
          m(I1, I0);
          if constexpr (NX == 2) rB(I0);
          m(I1, I1);
          if constexpr (NX == 2) rB(I1);
          m(I1, I2);
          if constexpr (NX == 2) rB(I2);
          rA(I1);
        }
        __builtin_amdgcn_sched_barrier(0);
      };
      kstep(QI<0>{}); kstep(QI<1>{}); kstep(QI<2>{}); kstep(QI<3>{});
      if constexpr (P == 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(6 + PA) : "memory");   // A0(t+1) has landed; the 6 + PA pieces requested since (P2, P3) stay in flight
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
    };
    // ONE loop body for every K-tile pair (no peeled last iteration: where the loop was split, hipcc shuffled accumulators between the register files
    // right behind MFMAs whose latency it cannot see -- whole 32x32 blocks came out stale). The last P4 of a tile therefore does its rolling reads as
    // well (K-tile 0 of the next tile, or a dead slot); they are not used: the next tile re-reads its first fragments after the epilogue.
    for (int kt = 0; kt < nk; kt += 2) {
      phase(QI<0>{}, QI<1>{}, QI<0>{}, kt); phase(QI<0>{}, QI<2>{}, QI<1>{}, kt); phase(QI<0>{}, QI<3>{}, QI<0>{}, kt); phase(QI<0>{}, QI<4>{}, QI<2>{}, kt);
      phase(QI<1>{}, QI<1>{}, QI<0>{}, kt + 1); phase(QI<1>{}, QI<2>{}, QI<1>{}, kt + 1); phase(QI<1>{}, QI<3>{}, QI<0>{}, kt + 1); phase(QI<1>{}, QI<4>{}, QI<2>{}, kt + 1);
    }
    // The MFMAs and fragment reads are inline asm: the distance between an MFMA's write and the first read of its result, and the landing of the last
    // (unused) rolling reads in registers the epilogue will reuse, are ours to keep. Every accumulator passes through this statement, so nothing that
    // reads one (the epilogue, a register-file shuffle of the allocator) can be placed in front of the wait states.
    if constexpr (MIH == 2) {
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_nop 15\n\ts_nop 15"
                   : "+a"(acc[0][0]), "+a"(acc[0][1]), "+v"(acc[0][2]), "+a"(acc[0][3]), "+a"(acc[0][4]), "+v"(acc[0][5]),
                     "+a"(acc[1][0]), "+a"(acc[1][1]), "+v"(acc[1][2]), "+a"(acc[1][3]), "+a"(acc[1][4]), "+v"(acc[1][5]),
                     "+a"(acc[2][0]), "+a"(acc[2][1]), "+v"(acc[2][2]), "+a"(acc[2][3]), "+a"(acc[2][4]), "+v"(acc[2][5]),
                     "+a"(acc[3][0]), "+a"(acc[3][1]), "+v"(acc[3][2]), "+a"(acc[3][3]), "+a"(acc[3][4]), "+v"(acc[3][5]));
    } else {
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_nop 15\n\ts_nop 15"
                   : "+a"(acc[0][0]), "+a"(acc[0][1]), "+v"(acc[0][2]), "+a"(acc[0][3]), "+a"(acc[0][4]), "+v"(acc[0][5]),
                     "+a"(acc[1][0]), "+a"(acc[1][1]), "+v"(acc[1][2]), "+a"(acc[1][3]), "+a"(acc[1][4]), "+v"(acc[1][5]));
    }
    stamp(2);
    float rscv[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) rscv[mi] = 1.0f;
    if constexpr (MIH == 1) {
      if (rs_on) {   // row wm * 64 + mi * 32 + l31 of the tile, summed in rms_row_scale's order
        int tl31 = l31;
        asm volatile("" : "+v"(tl31));
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          const float* q = reinterpret_cast<const float*>(smem + QC::RS_OFF) + (wm * (MI * 32) + mi * 32 + tl31) * 24;
          rscv[mi] = __builtin_amdgcn_rsqf(ln_tree24(q) * p.rs_invk + p.rs_eps);
        }
      }
    }
    q4_u32x4 rq[12];
    if constexpr (RSQ) {
      // the NEXT tile's partials travel across the epilogue from its second 32-row block on, in the registers of the first one's accumulators
      const int vq = nv >= 0 ? nv : cv;
      auto hook = [&](int mi) { if (mi == 1) rs_request(vq, rq); };
      tile_epilogue_256_impl<ACT, EPX, false, false, true, false, NI, MI>(p, acc, rsc, smem + QC::SLAB_OFF + w * 4096, lane, m0, n0, wm, wn, hook);
    } else {
      tile_epilogue_256<ACT, EPX, false, false, NI, MI>(p, acc, rscv, smem + QC::SLAB_OFF + w * 4096, lane, m0, n0, wm, wn);
    }
    stamp(3);
    __builtin_amdgcn_s_waitcnt(0xC07F);   // this wave's slab reads are done (the barrier at the top of the next tile frees the slot)
    cv = nv;
    if (cv < 0) break;
    aC = aN; wC = wN;
    nv = next_valid(cv + G);
    if (nv >= 0) tile_offs(nv, aN, wN);
    if constexpr (RSQ) rs_landed(QI<1>{}, rq);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the stream's trailing (unused) requests have landed before the LDS is released
}
