// Stand-alone host program around vima_amd/csrc/episode_book.h for tests/test_episode_book_build.py: one operation per line on stdin, one result
// line per operation on stdout. restart / install take one 0 / 1 flag per sample.
#include <iostream>
#include <sstream>
#include <string>

#include "episode_book.h"

int main() {
  EpisodeBook bk;
  static const char* const kind[] = {"legal", "full", "age", "long"};
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
    if (op == "begin") {
      int B, Q, P0, Lmax, ring;
      in >> B >> Q >> P0 >> Lmax >> ring;
      bk.begin(B, Q, P0, Lmax, ring != 0);
      out << "ok";
    } else if (op == "plan" || op == "step") {
      in >> T;
      const EpisodeBook::Plan p = bk.plan(T);
      if (p.refused) out << "refused " << kind[p.refused] << ' ' << p.sample << ' ' << p.fit << ' ' << p.age;
      else out << "plan " << p.row << ' ' << p.Lq << ' ' << p.advance << ' ' << p.Lk << ' ' << p.win_end << ' ' << p.hw;
      if (op == "step" && !p.refused) bk.commit(p, T);
    } else if (op == "restart") {
      bk.restart(flagged());
      out << "ok";
    } else if (op == "room") {
      out << "room " << bk.room();
    } else if (op == "rows" || op == "install") {   // like the library: a history beyond the room is refused before the book is asked
      in >> T;
      if (T < 1 || T > bk.room()) out << "refused room " << bk.room();
      else {
        std::vector<int> rows((size_t)T * (bk.Q + 1) - 1);
        const int age = bk.history_rows(T, rows.data());
        if (op == "install") bk.install(flagged(), age);
        out << op << ' ' << age;
        for (int r : rows) out << ' ' << r;
      }
    } else if (op == "left") {
      out << "left";
      for (int b = 0; b < bk.B; ++b) out << ' ' << bk.steps_left(b);
    } else if (op == "state") {
      out << "state " << bk.wp << ' ' << bk.hw << ' ' << bk.next << ' ' << bk.written_end() << ' ' << bk.slots.size() << " ages";
      for (int a : bk.age) out << ' ' << a;
    } else {
      out << "unknown operation " << op;
    }
    std::cout << out.str() << '\n';
  }
  return 0;
}
