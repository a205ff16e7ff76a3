// The host half of a resident tying (tying.hip): the checks pcl_tying_upload runs on a tree's node arrays before anything resident changes,
// and the two device layouts made from them.  Plain C++, no HIP: tests/tying_host_check.cpp compiles it alone and runs it on the CPU.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

// What ContextTree.Tree holds, with the meaning of the header's tree section: candidate c = pos * Q + qi (pos 0 left, 1 centre, 2 right),
// n_units = the utterance-edge symbol, node_child (N, 2) = (no, yes), nodes 0 .. R0 - 1 the roots, root_of (n_units P,).
struct TyingArrays {
    int n_units, P, Q;
    const uint8_t *q_member;     // (Q, n_units + 1)
    int N;
    const int32_t *node_cand;    // (N,) c, or -1 at a leaf
    const int32_t *node_child;   // (N, 2), or -1 at a leaf
    const int32_t *node_state;   // (N,) tied state at a leaf, -1 at an inner node
    int R0;
    const int32_t *root_of;      // (n_units P,)
    int J_t;
};

// One node of the walk: ONE 16-byte load per step.
struct TyingNode {
    int32_t cand, no, yes, state;
};

// 32-bit words per question in the bit table: bit u of row qi = q_member[qi][u], u in [0, n_units]
inline int tying_words(int n_units) { return (n_units + 1 + 31) / 32; }

// true when the arrays describe trees every walk of which ends in a leaf with a state in [0, J_t); otherwise false, and msg says which
// entry is wrong.  The order of the checks is the order of the header's list.
inline bool tying_validate(const TyingArrays &a, char *msg, size_t len) {
#define TY_BAD(...)                      \
    do {                                 \
        snprintf(msg, len, __VA_ARGS__); \
        return false;                    \
    } while (0)
    if (a.n_units < 1 || a.P < 1) TY_BAD("n_units = %d, P = %d", a.n_units, a.P);
    if (a.Q < 1 || 3LL * a.Q > 4096) TY_BAD("Q = %d questions (1 <= Q, 3 Q <= 4096)", a.Q);
    if (!a.q_member || !a.node_cand || !a.node_child || !a.node_state || !a.root_of) TY_BAD("NULL argument");
    if (a.N < 1 || a.R0 < 1 || a.R0 > a.N) TY_BAD("N = %d nodes, R0 = %d roots (1 <= R0 <= N)", a.N, a.R0);
    if (a.J_t < 1 || a.J_t > a.N) TY_BAD("J_t = %d tied states for %d nodes", a.J_t, a.N);
    std::vector<char> named((size_t)a.J_t, 0);
    int leaves = 0;
    for (int i = 0; i < a.N; ++i) {
        const int c = a.node_cand[i], no = a.node_child[2 * (size_t)i], yes = a.node_child[2 * (size_t)i + 1], st = a.node_state[i];
        if (c < 0) {                                               // a leaf
            if (c != -1) TY_BAD("node %d: candidate %d is neither -1 nor in [0, %d)", i, c, 3 * a.Q);
            if (no != -1 || yes != -1) TY_BAD("node %d is a leaf with children (%d, %d)", i, no, yes);
            if (st < 0 || st >= a.J_t) TY_BAD("node %d is a leaf with state %d outside [0, %d)", i, st, a.J_t);
            if (named[st]) TY_BAD("node %d: state %d is named by two leaves", i, st);
            named[st] = 1;
            ++leaves;
        } else {
            if (c >= 3 * a.Q) TY_BAD("node %d: candidate %d is neither -1 nor in [0, %d)", i, c, 3 * a.Q);
            // children behind their parent: a walk only ever moves to a larger node id, so it ends
            if (no <= i || no >= a.N || yes <= i || yes >= a.N) TY_BAD("node %d: children (%d, %d) outside (%d, %d)", i, no, yes, i, a.N);
            if (st != -1) TY_BAD("node %d is an inner node with state %d", i, st);
        }
    }
    if (leaves != a.J_t) TY_BAD("%d leaves for J_t = %d tied states", leaves, a.J_t);
    for (long long i = 0; i < (long long)a.n_units * a.P; ++i)
        if (a.root_of[i] < 0 || a.root_of[i] >= a.R0) TY_BAD("root_of[%lld] = %d outside [0, %d)", i, a.root_of[i], a.R0);
    return true;
#undef TY_BAD
}

// The two device layouts, from arrays tying_validate has accepted.
inline void tying_pack(const TyingArrays &a, std::vector<TyingNode> *nodes, std::vector<uint32_t> *qbits) {
    nodes->resize((size_t)a.N);
    for (int i = 0; i < a.N; ++i) (*nodes)[i] = TyingNode{a.node_cand[i], a.node_child[2 * (size_t)i], a.node_child[2 * (size_t)i + 1], a.node_state[i]};
    const int W = tying_words(a.n_units);
    qbits->assign((size_t)a.Q * W, 0u);
    for (int q = 0; q < a.Q; ++q)
        for (int u = 0; u <= a.n_units; ++u)
            if (a.q_member[(size_t)q * (a.n_units + 1) + u]) (*qbits)[(size_t)q * W + (u >> 5)] |= 1u << (u & 31);
}

// The walk itself, as the kernels run it (the host check holds it against a plain reading of the arrays).
inline int tying_walk_host(const TyingNode *nodes, const uint32_t *qbits, int Q, int W, int node, int left, int centre, int right) {
    for (;;) {
        const TyingNode nd = nodes[node];
        if (nd.cand < 0) return nd.state;
        const int pos = nd.cand / Q, qi = nd.cand - pos * Q;
        const int u = pos == 0 ? left : pos == 1 ? centre : right;
        node = (qbits[(size_t)qi * W + (u >> 5)] >> (u & 31)) & 1u ? nd.yes : nd.no;
    }
}
