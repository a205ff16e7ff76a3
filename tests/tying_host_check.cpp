// Host check of poccala_amd/csrc/tying_check.h: the validator pcl_tying_upload runs before anything resident changes, the packing of the
// two device layouts, and the walk over them against a plain reading of the arrays.  Plain C++, its own main, run on the CPU
// (tests/test_tied_twin.py builds it with the host's address and undefined-behaviour sanitizers).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../poccala_amd/csrc/tying_check.h"

static int fails = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            printf("FAILED line %d: %s\n", __LINE__, #x);            \
            ++fails;                                                 \
        }                                                            \
    } while (0)

struct Tree {
    int n_units = 3, P = 2, Q = 40, R0 = 2, J_t = 0;
    std::vector<uint8_t> qm;
    std::vector<int32_t> cand, child, state, root_of;
    TyingArrays arrays() const {
        return TyingArrays{n_units, P, Q, qm.data(), (int)cand.size(), cand.data(), child.data(), state.data(), R0, root_of.data(), J_t};
    }
};

// two shared roots (one per state position); root 0 splits twice, root 1 once; 40 questions over 4 symbols: 2 words a question would be
// needed from 32 symbols on, here one
static Tree good() {
    Tree t;
    t.qm.assign((size_t)t.Q * (t.n_units + 1), 0);
    for (int q = 0; q < t.Q; ++q)
        for (int u = 0; u <= t.n_units; ++u) t.qm[(size_t)q * (t.n_units + 1) + u] = (uint8_t)(((q * 7 + u * 3) % 5) < 2);
    //            0    1    2   3   4   5   6   7
    t.cand = {39, 2 * 40 + 5, -1, 40 + 3, -1, -1, -1, -1};
    t.child = {2, 3, 6, 7, -1, -1, 4, 5, -1, -1, -1, -1, -1, -1, -1, -1};
    t.state = {-1, -1, 0, -1, 1, 2, 3, 4};
    t.J_t = 5;
    t.root_of = {0, 1, 0, 1, 0, 1};
    return t;
}

static int plain_walk(const Tree &t, int l, int c, int r, int k) {
    int node = t.root_of[c * t.P + k];
    const int ctx[3] = {l, c, r};
    while (t.cand[node] >= 0) {
        const int pos = t.cand[node] / t.Q, qi = t.cand[node] % t.Q;
        node = t.child[2 * node + (t.qm[(size_t)qi * (t.n_units + 1) + ctx[pos]] ? 1 : 0)];
    }
    return t.state[node];
}

template <typename F>
static void refused(const char *what, F mutate) {
    Tree t = good();
    mutate(t);
    char msg[256] = "";
    const bool ok = tying_validate(t.arrays(), msg, sizeof(msg));
    printf("  %-28s -> %s\n", what, ok ? "ACCEPTED" : msg);
    CHECK(!ok && strlen(msg) > 0);
}

int main() {
    char msg[256] = "";
    Tree t = good();
    CHECK(tying_validate(t.arrays(), msg, sizeof(msg)));
    std::vector<TyingNode> nodes;
    std::vector<uint32_t> qbits;
    tying_pack(t.arrays(), &nodes, &qbits);
    const int W = tying_words(t.n_units);
    CHECK(W == 1 && tying_words(31) == 1 && tying_words(32) == 2 && tying_words(63) == 2 && tying_words(64) == 3);
    CHECK(nodes.size() == t.cand.size() && qbits.size() == (size_t)t.Q * W);
    int seen[5] = {0, 0, 0, 0, 0};
    for (int l = 0; l <= t.n_units; ++l)
        for (int c = 0; c < t.n_units; ++c)
            for (int r = 0; r <= t.n_units; ++r)
                for (int k = 0; k < t.P; ++k) {
                    const int want = plain_walk(t, l, c, r, k);
                    CHECK(tying_walk_host(nodes.data(), qbits.data(), t.Q, W, t.root_of[c * t.P + k], l, c, r) == want);
                    ++seen[want];
                }
    for (int s = 0; s < 5; ++s) CHECK(seen[s] > 0);              // every leaf is reached by some context
    // 40 units: two words a question, the edge symbol (40) in the second
    {
        Tree w = good();
        w.n_units = 40;
        w.qm.assign((size_t)w.Q * 41, 0);
        for (int q = 0; q < w.Q; ++q)
            for (int u = 0; u <= 40; ++u) w.qm[(size_t)q * 41 + u] = (uint8_t)(((q * 11 + u * 5) % 7) < 3);
        w.root_of.assign(40 * 2, 0);
        for (int i = 0; i < 80; ++i) w.root_of[i] = i % 2;
        CHECK(tying_validate(w.arrays(), msg, sizeof(msg)));
        tying_pack(w.arrays(), &nodes, &qbits);
        CHECK(tying_words(40) == 2 && qbits.size() == 80);
        for (int l = 0; l <= 40; l += 3)
            for (int r = 40; r >= 0; r -= 7)
                for (int c = 0; c < 40; c += 13)
                    for (int k = 0; k < 2; ++k)
                        CHECK(tying_walk_host(nodes.data(), qbits.data(), w.Q, 2, w.root_of[c * 2 + k], l, c, r) == plain_walk(w, l, c, r, k));
    }
    // 31, 32 and 96 units: the edge symbol at bit 31 of the only word, alone in the second word, alone in the fourth.  Every pair of
    // neighbours around centres at the word boundaries; root 0 asks the left neighbour about question Q - 1, the table's last row.
    for (int nu : {31, 32, 96}) {
        Tree w = good();
        w.n_units = nu;
        w.qm.assign((size_t)w.Q * (nu + 1), 0);
        for (int q = 0; q < w.Q; ++q)
            for (int u = 0; u <= nu; ++u) w.qm[(size_t)q * (nu + 1) + u] = (uint8_t)(((q * 11 + u * 5) % 7) < 3);
        w.qm[(size_t)(w.Q - 1) * (nu + 1) + nu] = 1;               // the edge symbol answers the last question: the last word is not zero
        w.root_of.assign((size_t)nu * 2, 0);
        for (int i = 0; i < nu * 2; ++i) w.root_of[i] = i % 2;
        CHECK(tying_validate(w.arrays(), msg, sizeof(msg)));
        tying_pack(w.arrays(), &nodes, &qbits);
        const int Ww = tying_words(nu);
        CHECK(Ww == (nu == 31 ? 1 : nu == 32 ? 2 : 4));
        CHECK(qbits.size() == (size_t)w.Q * Ww && qbits.back() != 0);
        if (nu != 31) CHECK(qbits.back() == 1u);                   // ... the edge symbol's bit and nothing beside it
        int walks = 0, edge_yes = 0;
        for (int c : {0, 30, 31, 32, 64, 95})
            if (c < nu)
                for (int l = 0; l <= nu; ++l)
                    for (int r = 0; r <= nu; ++r)
                        for (int k = 0; k < 2; ++k) {
                            const int want = plain_walk(w, l, c, r, k);
                            CHECK(tying_walk_host(nodes.data(), qbits.data(), w.Q, Ww, w.root_of[c * 2 + k], l, c, r) == want);
                            ++walks;
                            edge_yes += k == 0 && l == nu && want != 0;     // (state 0 is root 0's "no" leaf)
                        }
        CHECK(edge_yes > 0);
        printf("  %d units: W = %d, %zu words, last word %#x, %d walks\n", nu, Ww, qbits.size(), qbits.back(), walks);
    }
    // roots only
    {
        Tree r;
        r.P = 1;
        r.Q = 1;
        r.qm.assign(4, 0);
        r.cand = {-1, -1, -1};
        r.child = {-1, -1, -1, -1, -1, -1};
        r.state = {2, 0, 1};
        r.R0 = 3;
        r.J_t = 3;
        r.root_of = {0, 1, 2};
        CHECK(tying_validate(r.arrays(), msg, sizeof(msg)));
    }
    printf("refusals:\n");
    refused("child == its parent", [](Tree &x) { x.child[2 * 3] = 3; });
    refused("child < its parent", [](Tree &x) { x.child[2 * 3 + 1] = 1; });
    refused("child == N", [](Tree &x) { x.child[1] = 8; });
    refused("leaf state == J_t", [](Tree &x) { x.state[7] = 5; });
    refused("leaf state negative", [](Tree &x) { x.state[2] = -1; });
    refused("state named twice", [](Tree &x) { x.state[7] = 3; });
    refused("J_t larger than the leaves", [](Tree &x) { x.J_t = 6; });
    refused("cand == 3 Q", [](Tree &x) { x.cand[0] = 120; });
    refused("cand == -2", [](Tree &x) { x.cand[2] = -2; });
    refused("leaf with a child", [](Tree &x) { x.child[2 * 2] = 5; });
    refused("inner node with a state", [](Tree &x) { x.state[1] = 0; });
    refused("root_of == R0", [](Tree &x) { x.root_of[5] = 2; });
    refused("root_of negative", [](Tree &x) { x.root_of[0] = -1; });
    refused("R0 > N", [](Tree &x) { x.R0 = 9; });
    refused("Q == 0", [](Tree &x) { x.Q = 0; });
    refused("3 Q > 4096", [](Tree &x) { x.Q = 1366; });
    refused("P == 0", [](Tree &x) { x.P = 0; });
    if (fails) {
        printf("tying_host_check: %d FAILED\n", fails);
        return 1;
    }
    printf("tying_host_check: OK\n");
    return 0;
}
