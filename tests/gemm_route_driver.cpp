// Stand-alone host program around vima_amd/csrc/gemm_route.h (tests/test_gemm_route_build.py compiles it with a host compiler under
// AddressSanitizer + UndefinedBehaviorSanitizer and runs it as a child process). One line of stdin per question, one line of stdout per answer:
//   R ncu is_bf16 <15 knobs> <7 strides> <25 ints> <17 pointers: byte offset from a 256-byte boundary, -1 = null>   ->   "<0|invalid|other> <kernel_id>"
//   P <15 knobs> M N K lda ldw <hm_D hm_L>...                                                     ->   one 0/1 per predicate column
// in the field orders of tests/gemm_route_cases.py (KNOBS, I64, I32, PTRS, PREDICATES). Pointers are made-up addresses: the route never reads them.
#include <stdio.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gemm_route.h"

using namespace vima;

static Tuning read_knobs(std::istream& in) {
  Tuning t;
  int* f[15] = {&t.gemm_variant, &t.gemm_tile, &t.gemm_raster, &t.gemm_epi, &t.gemm_persist, &t.gemm_small, &t.gemm_wide, &t.gemm_pp, &t.gemm_q4, &t.gemm_splitk,
                &t.gemm_resident, &t.gemm_res_maxwg, &t.gemm_skinny, &t.gemm_flat, &t.gemm_res_nch};
  for (int* p : f) in >> *p;
  return t;
}

template <typename P>
static void read_ptr(std::istream& in, int slot, P& p) {
  long long off;
  in >> off;
  p = off < 0 ? nullptr : reinterpret_cast<P>((uintptr_t)(slot + 1) * (1u << 28) + (uintptr_t)off);
}

static std::string route_line(std::istream& in) {
  int ncu, is_bf16;
  in >> ncu >> is_bf16;
  const Tuning t = read_knobs(in);
  GemmArgs a;
  a.tune = &t;
  in >> a.bsA >> a.bsW >> a.bsBias >> a.bsMul >> a.bsRes >> a.bs32 >> a.bsT;
  in >> a.M >> a.N >> a.K >> a.lda >> a.ldw >> a.lda2 >> a.ldw2 >> a.ldmul >> a.ldres >> a.ldresT >> a.ld32 >> a.ldT >> a.ldT_lo >> a.batch >> a.act;
  in >> a.hm_D >> a.hm_L >> a.pair32 >> a.rb >> a.s_hi >> a.s_lo >> a.ro >> a.split_n >> a.rs_parts >> a.x3;
  int s = 0;
  read_ptr(in, s++, a.A); read_ptr(in, s++, a.W); read_ptr(in, s++, a.A2); read_ptr(in, s++, a.W2); read_ptr(in, s++, a.mul); read_ptr(in, s++, a.resT);
  read_ptr(in, s++, a.outT); read_ptr(in, s++, a.outT_lo); read_ptr(in, s++, a.bias); read_ptr(in, s++, a.res); read_ptr(in, s++, a.rs_ssq);
  read_ptr(in, s++, a.rs_sum); read_ptr(in, s++, a.rs_c); read_ptr(in, s++, a.out32); read_ptr(in, s++, a.ssq_out); read_ptr(in, s++, a.sum_out);
  read_ptr(in, s++, a.grp_col);
  if (!in) return "bad line";
  // the split-K scratch the way vima_op_gemm brings it: whatever the plan asks for
  const SplitPlan sp = splitk_plan(a, is_bf16 != 0);
  if (sp.S > 1) { a.splitk_ws = reinterpret_cast<float*>(uintptr_t(20) << 28); a.splitk_ws_bytes = (size_t)sp.S * a.M * a.N * sizeof(float); }
  const GemmRoute r = gemm_route(a, is_bf16 != 0, ncu);
  return std::string(r.err == 0 ? "0" : (r.err == kGemmInvalid ? "invalid" : "other")) + " " + std::to_string(r.kernel_id);
}

static std::string predicate_line(std::istream& in) {
  const Tuning t = read_knobs(in);
  long long M, N, K, lda, ldw;
  in >> M >> N >> K >> lda >> ldw;
  const int ncu = 256;
  std::string out;
  const auto put = [&out](int v) { out += v ? '1' : '0'; };
  put(route_q::pair_large(&t, M, N, K, ncu));
  put(route_q::pair_ok(&t, M, N, K, ncu));
  put(route_q::lnfold_producer_ok(&t, M, N, ncu));
  put(route_q::dual_ok(&t, (int)M, (int)N, ncu));
  put(route_q::a8_ok(&t, M, N, K, lda, ldw, ncu));
  put(route_q::grouped_ok(&t, ncu));
  int D, L;
  while (in >> D >> L)
    for (int a8 = 0; a8 < 2; ++a8) put(route_q::headmajor_ok(&t, M, N, K, lda, ldw, D, L, a8, ncu));
  return out;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind;
    in >> kind;
    puts((kind == "R" ? route_line(in) : kind == "P" ? predicate_line(in) : std::string("bad line")).c_str());
  }
  return 0;
}
