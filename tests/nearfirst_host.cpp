// Host model of the near-first fold (csrc/rt_math.h: nf_pass_bound, nf_near_tie, the
// functions cast_local itself calls).  A lane meets the leaves its ray hits in some order; each
// candidate is a leaf's inside-passing triangle with local time tt.  The reference folds them in
// DFS order: accept when tt < B, then B = (tt * scale) * dir_len.  The near-first walk folds them
// in another order with the widened plane compare and the near-tie flag.  Checked here, for every
// visiting order of random candidate sets (times far apart, exactly equal, 1-16 ulps apart; scale
// and dir_len 1 or 1 +- 1 ulp): either the flag is raised, or winner and converted time equal the
// DFS fold's.  And far-apart sets raise no flag in any order.
// Prints "sets orders flagged unflagged_checked far_sets"; exit status 1 on a counterexample.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "rt_math.h"

namespace {

struct Fold { int winner; float best; bool flag; };

float conv(float tt, float scale, float dir_len) { return (tt * scale) * dir_len; }   // fix_isect, then cast_local

// the reference's fold, in the order given (DFS order: the identity)
Fold fold_dfs(const std::vector<float>& tt, float scale, float dir_len) {
    Fold f{-1, INFINITY, false};
    for (int i = 0; i < (int)tt.size(); i++)
        if (tt[i] < f.best) { f.best = conv(tt[i], scale, dir_len); f.winner = i; }
    return f;
}

// the near-first walk's fold over leaves visited in `order` (one candidate per leaf: cast_local's
// first triangle of a visit, the only one compared against the widened entry best)
Fold fold_near(const std::vector<float>& tt, const std::vector<int>& order, float scale, float dir_len) {
    Fold f{-1, INFINITY, false};
    for (int i : order) {
        const float t_entry = f.best;
        if (!(tt[i] < rtm::nf_pass_bound(t_entry))) continue;          // the plane compare
        if (rtm::nf_near_tie(tt[i], t_entry)) f.flag = true;
        if (tt[i] < t_entry) { f.best = conv(tt[i], scale, dir_len); f.winner = i; }
    }
    return f;
}

float ulps(float x, int k) {
    int32_t b;
    memcpy(&b, &x, 4);
    b += k;
    memcpy(&x, &b, 4);
    return x;
}

}  // namespace

int main() {
    std::mt19937 rng(12345);
    std::uniform_real_distribution<float> ut(0.5f, 900.0f);
    long sets = 0, orders = 0, flagged = 0, checked = 0, far_sets = 0;
    const float one[3] = {1.0f, ulps(1.0f, 1), ulps(1.0f, -1)};
    for (int it = 0; it < 20000; it++) {
        const int n = 2 + (int)(rng() % 5);
        const int kind = (int)(rng() % 4);                     // 0 far apart, 1 equal pairs, 2 within 16 ulps, 3 mixed
        std::vector<float> tt(n);
        const float base = ut(rng);
        for (int i = 0; i < n; i++) {
            const int k = kind == 3 ? (int)(rng() % 3) : kind;
            if (k == 0 || i == 0) tt[i] = kind == 0 ? base * (1.0f + 0.01f * (float)(i + 1) * (float)(1 + rng() % 7)) : ut(rng);
            else if (k == 1) tt[i] = tt[rng() % i];
            else tt[i] = ulps(tt[rng() % i], (int)(rng() % 33) - 16);
        }
        if (kind == 0) std::shuffle(tt.begin(), tt.end(), rng);
        bool far = true;                                       // every pair further apart than 2^-18 relative
        for (int i = 0; i < n; i++)
            for (int j = 0; j < i; j++) far = far && std::fabs(tt[i] - tt[j]) > 0x1p-18f * std::fmax(tt[i], tt[j]);
        for (float scale : one)
            for (float dir_len : one) {
                const Fold d = fold_dfs(tt, scale, dir_len);
                std::vector<int> order(n);
                for (int i = 0; i < n; i++) order[i] = i;
                sets++;
                far_sets += far;
                do {
                    const Fold f = fold_near(tt, order, scale, dir_len);
                    orders++;
                    if (f.flag) {
                        flagged++;
                        if (far) { printf("flag on a far-apart set (n = %d, base %a)\n", n, tt[0]); return 1; }
                        continue;
                    }
                    checked++;
                    if (f.winner != d.winner || memcmp(&f.best, &d.best, 4) != 0) {
                        printf("unflagged order differs: n = %d winner %d / %d time %a / %a scale %a dir_len %a\n", n, f.winner,
                               d.winner, f.best, d.best, scale, dir_len);
                        for (int i = 0; i < n; i++) printf("  tt[%d] = %a (order %d)\n", i, tt[i], order[i]);
                        return 1;
                    }
                } while (std::next_permutation(order.begin(), order.end()));
            }
    }
    printf("%ld %ld %ld %ld %ld\n", sets, orders, flagged, checked, far_sets);
    return flagged > 0 && checked > 0 && far_sets > 0 ? 0 : 1;
}
