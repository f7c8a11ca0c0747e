// Host bookkeeping of an episode cache: which cache rows the next env steps of a batch write, and which may be overwritten. Plain C++17, no HIP:
// tests/episode_book_driver.cpp holds it on the CPU against the Python restatements (units, forks, snapshots).
//
// Rows [0, P0) of every sample's cache block are a fixed prefix (P0 = 0 for the XAttnGPT policies, prompt + separator for GPT / Gato); the rows
// [P0, Lmax) behind it are ONE row index space for the whole batch, linear or a ring (options decode_ring / seq_ring). A call of T env steps is one
// unit of Lq = T (Q + 1) rows -- T slots of [action row, Q obs rows]; the first slot of batch step 0 has no action row -- and is never split across
// the wrap: when it does not fit in front of Lmax, the tail [wp, Lmax) is skipped (and counts as advanced) and the rows go to [P0, P0 + Lq).
// Ring: a unit is legal iff every row it overwrites or skips is dead for every sample, age[b] + advance <= Lmax - P0.
#pragma once
#include <algorithm>
#include <vector>

struct EpisodeBook {
  enum Refusal { LEGAL = 0, FULL, OVER_AGE, TOO_LONG };   // the linear cache is full; ring: sample `sample` is over age; the unit is longer than the ring
  // row: first cache row the unit writes; Lk / win_end: keys its self-attention reads and the end of its causal window (0: the plain rule); hw: the
  // high-water mark after it. Refused: the offender (FULL / TOO_LONG: sample 0), its age, and how many single steps still fit for it
  struct Plan { int row, Lq, advance, Lk, win_end, hw; Refusal refused; int sample, age, fit; };
  // per batch step: its first obs row (its action row, absent at batch step 0, is obs_row - 1) and the rows it advanced (a chunk's skipped tail
  // counts with its first slot)
  struct Slot { int obs_row, adv; };

  int B = 0, Q = 0, P0 = 0, Lmax = 0;
  bool ring = false;
  int wp = 0;                // next row to write (linear: the rows in use)
  int hw = 0;                // one past the highest row written since begin() (rows beyond it hold garbage and are never read)
  int next = 0;              // the batch step the next unit starts with
  std::vector<int> age;      // per sample: rows advanced (skipped tails included) since its episode began
  std::vector<Slot> slots;   // the last batch steps, at most Lmax of them (a step advances at least one row)

  void begin(int B_, int Q_, int P0_, int Lmax_, bool ring_) {
    B = B_; Q = Q_; P0 = P0_; Lmax = Lmax_; ring = ring_;
    wp = hw = P0; next = 0;
    age.assign((size_t)B, 0); slots.clear();
  }

  Plan plan(int T) const {
    Plan p{};
    const long long Lq = (long long)T * (Q + 1) - (next == 0 ? 1 : 0);
    if (ring ? Lq > Lmax - P0 : wp + Lq > Lmax) return refuse(p, ring ? TOO_LONG : FULL, 0);
    p.Lq = (int)Lq;
    p.advance = place(wp, p.Lq, p.row);
    for (int b = 0; b < B; ++b)
      if (!alive(age[b], wp, p.Lq, p.advance)) return refuse(p, OVER_AGE, b);
    p.win_end = ring ? p.row + p.Lq : 0;
    p.hw = std::max(hw, p.row + p.Lq);
    p.Lk = ring ? p.hw : p.row + p.Lq;
    return p;
  }

  void commit(const Plan& p, int T) {
    for (int& a : age) a += p.advance;
    for (int u = 0; u < T; ++u) slots.push_back({p.row + u * (Q + 1) + (next > 0 ? 1 : 0), u == 0 ? p.advance - (T - 1) * (Q + 1) : Q + 1});
    if ((int)slots.size() > Lmax) slots.erase(slots.begin(), slots.end() - Lmax);
    wp = p.row + p.Lq; hw = p.hw; next += T;
  }

  // the listed samples' rows are dead: later units may overwrite them (a restart itself takes no rows)
  void restart(const std::vector<int>& list) { install(list, 0); }

  // The largest history that can be installed now: the last batch steps whose rows are all still there, i.e. whose advances sum to at most the row
  // space (a sample restarted right before them would still be legal now). Linear: every step since begin()
  int room() const {
    int r = 0, sum = 0;
    for (int j = (int)slots.size() - 1; j >= 0 && sum + slots[j].adv <= Lmax - P0; --j) { sum += slots[j].adv; ++r; }
    return r;
  }

  // Cache rows of the T (Q + 1) - 1 compact rows [o_0 (Q), a_0, o_1 (Q), ...] of a history of T <= room() steps: step s goes in the slot of batch
  // step next - T + s, its action in the NEXT slot's action row. Returns the age of a sample restarted right before those steps
  int history_rows(int T, int* out) const {
    const Slot* S = slots.data() + (slots.size() - (size_t)T);
    int a = 0;
    for (int s = 0; s < T; ++s) {
      a += S[s].adv;
      for (int q = 0; q < Q; ++q) *out++ = S[s].obs_row + q;
      if (s + 1 < T) *out++ = S[s + 1].obs_row - 1;
    }
    return a;
  }

  void install(const std::vector<int>& list, int a) { for (int b : list) age[(size_t)b] = a; }

  // A history of the last T batch steps as every entry installs it (restart with a history, snapshot, restore). fits: the room rule, 0 <= T <=
  // room -- nothing else is filled when it fails. rows: [the identity over the prefix [0, P0), when asked | history_rows(T)]; age: what
  // history_rows returns (T = 0: 0). in_range: every history row lies in [P0, written_end()) -- a batch step wrote each of them, so a row outside
  // is an error of this book
  struct History { bool fits, in_range; int room, age; std::vector<int> rows; };
  History history(int T, bool with_prefix) const {
    History H{false, true, room(), 0, {}};
    H.fits = T >= 0 && T <= H.room;
    if (!H.fits) return H;
    const int P = with_prefix ? P0 : 0, R = std::max(T * (Q + 1) - 1, 0);
    H.rows.resize((size_t)P + R);
    for (int l = 0; l < P; ++l) H.rows[(size_t)l] = l;
    if (T > 0) H.age = history_rows(T, H.rows.data() + P);
    for (int l = P; l < P + R; ++l) H.in_range = H.in_range && H.rows[(size_t)l] >= P0 && H.rows[(size_t)l] < written_end();
    return H;
  }

  // Episode snapshots: the number n of env steps sample b's episode has taken -- the trailing slots whose advances sum to age[b] exactly (0 right
  // after a restart); history_rows(n, .) then lists the episode's rows in compact time order. -1 when no suffix of the slot record sums to the age
  // (the record was trimmed below the episode, which a legal ring never does). A snapshot is restored by install(list, history_rows(n, .)) on the
  // book of that later moment, under the rule of every installed history: n <= room()
  int steps_of(int b) const {
    const int a = age[(size_t)b];
    int n = 0, sum = 0;
    for (int j = (int)slots.size() - 1; j >= 0 && sum < a; --j) { sum += slots[j].adv; ++n; }
    return sum == a ? n : -1;
  }

  // how many further single steps would succeed if sample b alone were never restarted: the single-step plan run forward
  int steps_left(int b) const {
    int n = 0, w = wp, a = age[(size_t)b], row = 0;
    for (int Lq = Q + (next > 0 ? 1 : 0);; Lq = Q + 1, ++n) {
      const int adv = place(w, Lq, row);
      if (!alive(a, w, Lq, adv)) return n;
      a += adv; w = row + Lq;
    }
  }

  int written_end() const { return ring ? hw : wp; }   // one past the last row that may hold a live key

  // Fork: slot b continues the episode of slot source[b] (source[b] == b: untouched). Legal iff every entry is a sample and every source is its own
  // source -- no chains, no swaps -- so that the copy runs in place without ordering hazards: no slot is both read and written
  bool fork_ok(const std::vector<int>& source) const {
    if ((int)source.size() != B) return false;
    for (int s : source)
      if (s < 0 || s >= B || source[(size_t)s] != s) return false;
    return true;
  }

  // the destination takes its source's age (its old episode is dropped, as in restart); everything else is batch-wide
  void fork(const std::vector<int>& source) {
    for (int b = 0; b < B; ++b) age[(size_t)b] = age[(size_t)source[(size_t)b]];
  }

  // At most two disjoint half-open row ranges inside [P0, written_end()) that hold every row sample b's episode has written and that is still
  // there: the last age[b] advanced rows behind wp. Ring: where they reach back beyond P0, [P0, wp) and the rest counted back from Lmax, cut at hw
  // (rows of a skipped tail beyond hw were never written). -> the number of ranges; their lengths sum to at most age[b]
  int live_ranges(int b, int out[2][2]) const {
    const int a = age[(size_t)b];
    int n = 0;
    auto put = [&](int lo, int hi) { if (lo < hi) { out[n][0] = lo; out[n][1] = hi; ++n; } };
    if (a <= 0) return 0;
    if (!ring || wp - a >= P0) { put(std::max(P0, wp - a), wp); return n; }
    put(P0, wp);
    put(std::max(wp, Lmax - (a - (wp - P0))), hw);
    return n;
  }

 private:
  int place(int w, int Lq, int& row) const {   // -> rows advanced
    const bool wrap = w + Lq > Lmax;
    row = wrap ? P0 : w;
    return wrap ? Lmax - w + Lq : Lq;
  }
  bool alive(int a, int w, int Lq, int adv) const { return ring ? a + adv <= Lmax - P0 : w + Lq <= Lmax; }
  Plan refuse(Plan p, Refusal why, int b) const {
    p.refused = why; p.sample = b; p.age = age[(size_t)b]; p.fit = steps_left(b);
    return p;
  }
};
