// Stand-alone host program around vima_amd/csrc/episode_book.h for tests/test_episode_snapshot_build.py: one operation per line on stdin, one result
// line per operation on stdout. The operations of tests/episode_fork_driver.cpp plus the snapshot bookkeeping: `snap b` = steps_of + history_rows,
// `restore n d ..` = the room rule, history_rows on the current book and install per slot -- what vima_decode_snapshot / vima_decode_restore do
// on the host.
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
    auto rows_of = [&](int n, int& age) {   // the compact -> cache row map of the last n batch steps
      std::vector<int> rows((size_t)std::max(n * (bk.Q + 1) - 1, 0));
      age = n > 0 ? bk.history_rows(n, rows.data()) : 0;
      return rows;
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
        int age = 0;
        rows_of(T, age);
        bk.install(flagged(), age);
        out << "install " << age;
      }
    } else if (op == "fork") {
      const std::vector<int> source = ints();
      if (!bk.fork_ok(source)) out << "refused";
      else {
        bk.fork(source);
        out << "ok";
      }
    } else if (op == "snap") {   // `snap n | rows` of sample b, or `snap -1`
      int b = 0;
      in >> b;
      const int n = bk.steps_of(b);
      out << "snap " << n;
      if (n >= 0 && n <= bk.room()) {
        int age = 0;
        out << " |";
        for (int r : rows_of(n, age)) out << ' ' << r;
      }
    } else if (op == "restore") {   // a snapshot of n steps into the listed slots: `restore age | rows`, or `refused room r`
      int n = 0;
      in >> n;
      const std::vector<int> slots = ints();
      if (n < 0 || n > bk.room()) out << "refused room " << bk.room();
      else {
        int age = 0;
        const std::vector<int> rows = rows_of(n, age);
        for (int d : slots) bk.install(std::vector<int>{d}, age);
        out << "restore " << age << " |";
        for (int r : rows) out << ' ' << r;
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
