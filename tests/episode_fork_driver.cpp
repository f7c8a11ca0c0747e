// Stand-alone host program around vima_amd/csrc/episode_book.h for tests/test_episode_fork_build.py: one operation per line on stdin, one result
// line per operation on stdout. restart / install take one 0 / 1 flag per sample, fork / forkok one source per sample (forkok: any number).
#include <iostream>
#include <sstream>
#include <string>

#include "episode_book.h"

int main() {
  EpisodeBook bk;
  std::string line, op;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::ostringstream out;
    int T = 0;
    in >> op;
    auto flagged = [&] {
      std::vector<int> list;
      for (int b = 0, f; b < bk.B && in >> f; ++b)
        if (f) list.push_back(b);
      return list;
    };
    auto ints = [&] {
      std::vector<int> v;
      for (int x; in >> x;) v.push_back(x);
      return v;
    };
    if (op == "begin") {
      int B, Q, P0, Lmax, ring;
      in >> B >> Q >> P0 >> Lmax >> ring;
      bk.begin(B, Q, P0, Lmax, ring != 0);
      out << "ok";
    } else if (op == "step") {
      in >> T;
      const EpisodeBook::Plan p = bk.plan(T);
      if (p.refused) out << "refused";
      else {
        bk.commit(p, T);
        out << "plan " << p.row << ' ' << p.Lq << ' ' << p.advance;
      }
    } else if (op == "restart") {
      bk.restart(flagged());
      out << "ok";
    } else if (op == "install") {
      in >> T;
      if (T < 1 || T > bk.room()) out << "refused room " << bk.room();
      else {
        std::vector<int> rows((size_t)T * (bk.Q + 1) - 1);
        const int age = bk.history_rows(T, rows.data());
        bk.install(flagged(), age);
        out << "install " << age;
      }
    } else if (op == "forkok") {
      out << "forkok " << (bk.fork_ok(ints()) ? 1 : 0);
    } else if (op == "fork") {
      const std::vector<int> source = ints();
      if (!bk.fork_ok(source)) out << "refused";
      else {
        bk.fork(source);
        out << "ok";
      }
    } else if (op == "ranges") {   // of every sample: `ranges | lo hi [lo hi] | ...`
      out << "ranges";
      for (int b = 0; b < bk.B; ++b) {
        int r[2][2];
        const int n = bk.live_ranges(b, r);
        out << " |";
        for (int i = 0; i < n; ++i) out << ' ' << r[i][0] << ' ' << r[i][1];
      }
    } else if (op == "left") {
      out << "left";
      for (int b = 0; b < bk.B; ++b) out << ' ' << bk.steps_left(b);
    } else if (op == "state") {
      out << "state " << bk.wp << ' ' << bk.hw << ' ' << bk.next << ' ' << bk.written_end() << " ages";
      for (int a : bk.age) out << ' ' << a;
    } else {
      out << "unknown operation " << op;
    }
    std::cout << out.str() << '\n';
  }
  return 0;
}
