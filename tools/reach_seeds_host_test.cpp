// Host harness of the reach seeds rule (csrc/reach_seeds.hpp), compiled with
// the host compiler alone (tests/test_reach_seeds_host.py).
//   stdin, one case per line:
//     "w" rule S, then per seed: result steps e_p e_R   -> the winner's index
//     "k" rule S k s                                    -> the key, as an integer
//     "c" rule S word k s                               -> 0 / 1: the cancel predicate
//     "i" rule S K  -> the interleaving check: for every assignment of
//         uncancelled outcomes (REACHED or not, stopping at step 0 .. K) to S
//         seeds, every order in which the seeds' steps can interleave and every
//         value a read of the group's word can return (the present one or any it
//         held before, the initial one included).  Prints the number of complete
//         schedules, how many cancelled a seed, and the violations: schedules in
//         which the true winner stopped as CANCELLED, or whose outcomes give
//         seeds_winner another seed, step count or result.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../dyros_robot_controller_amd/csrc/reach_seeds.hpp"

using namespace drc_amd;

namespace {

struct Sim {
  int rule, S, K;
  int reach[4], stop[4];  // uncancelled: REACHED or not, at which step
  int true_win;
  int pos[4], done[4], res[4], steps[4];
  std::vector<uint32_t> hist;  // the word's values, oldest first
  long long leaves = 0, cancels = 0, bad = 0;

  void leaf() {
    ++leaves;
    int32_t r[4], st[4];
    double ep[4], er[4];
    bool any = false;
    for (int s = 0; s < S; ++s) {
      r[s] = res[s];
      st[s] = steps[s];
      ep[s] = 1.0 + ((s * 7 + stop[s]) % 3);  // (used only if none reached: then nothing is cancelled)
      er[s] = 0.5;
      any |= res[s] == kSeedsCancelled;
    }
    cancels += any;
    const int w = seeds_winner(rule, S, r, st, ep, er, 1);
    const int want_res = reach[true_win] ? kSeedsReached : 1;
    if (w != true_win || st[w] != stop[true_win] || r[w] != want_res) ++bad;
  }

  void run() {
    int live = -1;
    for (int s = 0; s < S; ++s)
      if (!done[s]) live = s;
    if (live < 0) return leaf();
    for (int s = 0; s < S; ++s) {
      if (done[s]) continue;
      const int k = pos[s];
      if (k == stop[s]) {  // its last step: publish or stop on its own
        done[s] = 1;
        res[s] = reach[s] ? kSeedsReached : 1;
        steps[s] = k;
        const size_t n = hist.size();
        if (reach[s]) {
          const uint32_t key = seeds_key(rule, S, k, s);
          if (key < hist.back()) hist.push_back(key);
        }
        run();
        hist.resize(n);
        done[s] = 0;
        continue;
      }
      // outside the tolerances with steps left: read the word, fresh or stale
      for (size_t h = 0; h < hist.size(); ++h) {
        if (seeds_cancelled(rule, S, hist[h], k, s)) {
          if (s == true_win) ++bad;
          done[s] = 1;
          res[s] = kSeedsCancelled;
          steps[s] = k;
          run();
          done[s] = 0;
        } else {
          pos[s] = k + 1;
          run();
          pos[s] = k;
        }
      }
    }
  }

  void all(int s) {
    if (s == S) {
      int32_t r[4], st[4];
      double ep[4], er[4];
      for (int i = 0; i < S; ++i) {
        r[i] = reach[i] ? kSeedsReached : 1;
        st[i] = stop[i];
        ep[i] = 1.0 + ((i * 7 + stop[i]) % 3);
        er[i] = 0.5;
        pos[i] = done[i] = 0;
      }
      true_win = seeds_winner(rule, S, r, st, ep, er, 1);
      hist.assign(1, kSeedsNoKey);
      run();
      return;
    }
    for (reach[s] = 0; reach[s] < 2; ++reach[s])
      for (stop[s] = 0; stop[s] <= K; ++stop[s]) all(s + 1);
  }
};

}  // namespace

int main() {
  char kind;
  while (std::scanf(" %c", &kind) == 1) {
    int rule, S;
    if (std::scanf("%d %d", &rule, &S) != 2 || S < 1) return 1;
    if (kind == 'w') {
      std::vector<int32_t> r(S), st(S);
      std::vector<double> ep(S), er(S);
      for (int s = 0; s < S; ++s)
        if (std::scanf("%" SCNd32 " %" SCNd32 " %lf %lf", &r[s], &st[s], &ep[s], &er[s]) != 4) return 1;
      std::printf("%d\n", seeds_winner(rule, S, r.data(), st.data(), ep.data(), er.data(), 1));
    } else if (kind == 'k') {
      int k, s;
      if (std::scanf("%d %d", &k, &s) != 2) return 1;
      std::printf("%" PRIu32 "\n", seeds_key(rule, S, k, s));
    } else if (kind == 'c') {
      uint32_t word;
      int k, s;
      if (std::scanf("%" SCNu32 " %d %d", &word, &k, &s) != 3) return 1;
      std::printf("%d\n", seeds_cancelled(rule, S, word, k, s) ? 1 : 0);
    } else if (kind == 'i') {
      Sim sim{};
      sim.rule = rule;
      sim.S = S;
      if (std::scanf("%d", &sim.K) != 1 || S > 4) return 1;
      sim.all(0);
      std::printf("%lld %lld %lld\n", sim.leaves, sim.cancels, sim.bad);
    } else {
      return 1;
    }
  }
  return 0;
}
