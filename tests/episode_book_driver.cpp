// Stand-alone host program around vima_amd/csrc/episode_book.h for tests/test_episode_book_build.py, test_episode_fork_build.py and
// test_episode_snapshot_build.py (built by tests/episode_driver.py): one operation per line on stdin, one result line per operation on stdout.
// restart / install take one 0 / 1 flag per sample, fork / forkok one source per sample (forkok: any number), restore its slots. Every history
// (rows, install, hist, snap, restore) is EpisodeBook::history, the member the library's entries call: the room rule, the table, the age, the range
// check. With an argument (`brief`) plan / step, install and state print the short lines of the fork and snapshot tests.
#include <iostream>
#include <sstream>
#include <string>

#include "episode_book.h"

int main(int argc, char**) {
  const bool brief = argc > 1;
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
    auto ints = [&] {
      std::vector<int> v;
      for (int x; in >> x;) v.push_back(x);
      return v;
    };
    // like the library: a history beyond the room is refused; a row outside [P0, written_end()) would be its internal error
    auto refused = [&](const EpisodeBook::History& H) {
      if (!H.fits) out << "refused room " << H.room;
      else if (!H.in_range) out << "internal error: history row outside the written cache";
      return !H.fits || !H.in_range;
    };
    auto rows = [&](const EpisodeBook::History& H) {
      for (int r : H.rows) out << ' ' << r;
    };
    if (op == "begin") {
      int B, Q, P0, Lmax, ring;
      in >> B >> Q >> P0 >> Lmax >> ring;
      bk.begin(B, Q, P0, Lmax, ring != 0);
      out << "ok";
    } else if (op == "plan" || op == "step") {
      in >> T;
      const EpisodeBook::Plan p = bk.plan(T);
      if (p.refused) out << "refused";
      else out << "plan " << p.row << ' ' << p.Lq << ' ' << p.advance;
      if (p.refused && !brief) out << ' ' << kind[p.refused] << ' ' << p.sample << ' ' << p.fit << ' ' << p.age;
      if (!p.refused && !brief) out << ' ' << p.Lk << ' ' << p.win_end << ' ' << p.hw;
      if (op == "step" && !p.refused) bk.commit(p, T);
    } else if (op == "restart") {
      bk.restart(flagged());
      out << "ok";
    } else if (op == "room") {
      out << "room " << bk.room();
    } else if (op == "rows" || op == "install") {
      in >> T;
      const EpisodeBook::History H = bk.history(std::max(T, 0), false);
      if (T < 1) out << "refused room " << H.room;
      else if (!refused(H)) {
        if (op == "install") bk.install(flagged(), H.age);
        out << op << ' ' << H.age;
        if (op == "rows" || !brief) rows(H);
      }
    } else if (op == "hist") {   // the table behind the identity over the prefix: `hist age | rows`
      in >> T;
      const EpisodeBook::History H = bk.history(T, true);
      if (!refused(H)) {
        out << "hist " << H.age << " |";
        rows(H);
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
    } else if (op == "snap") {   // `snap n | rows` of sample b, or `snap -1`
      int b = 0;
      in >> b;
      const int n = bk.steps_of(b);
      out << "snap " << n;
      const EpisodeBook::History H = bk.history(n, false);
      if (H.fits) {
        out << " |";
        if (!refused(H)) rows(H);
      }
    } else if (op == "restore") {   // a snapshot of n steps into the listed slots: `restore age | rows`, or `refused room r`
      int n = 0;
      in >> n;
      const std::vector<int> slots = ints();
      const EpisodeBook::History H = bk.history(n, false);
      if (!refused(H)) {
        bk.install(slots, H.age);
        out << "restore " << H.age << " |";
        rows(H);
      }
    } else if (op == "left") {
      out << "left";
      for (int b = 0; b < bk.B; ++b) out << ' ' << bk.steps_left(b);
    } else if (op == "state") {
      out << "state " << bk.wp << ' ' << bk.hw << ' ' << bk.next << ' ' << bk.written_end();
      if (!brief) out << ' ' << bk.slots.size();
      out << " ages";
      for (int a : bk.age) out << ' ' << a;
    } else {
      out << "unknown operation " << op;
    }
    std::cout << out.str() << '\n';
  }
  return 0;
}
