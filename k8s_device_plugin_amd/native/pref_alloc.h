// Native preferred-allocation search: the same best-effort policy as
// allocator/besteffort.py (grouping, anti-fragmentation ordering, seed +
// breadth-first extension with parent-set dedup, first strict minimum),
// written once and parametrised by how a group's nodes are scored.
//
// Host-only and standard-library-only, so tests/native/pref_alloc_check.cpp
// can run it as a stand-alone program under the sanitizers; fastserver.cpp
// calls it from the GetPreferredAllocation handler.
#pragma once

#include <algorithm>
#include <cstdint>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <unordered_map>
#include <utility>
#include <vector>

namespace prefalloc {

struct AllocState {
    std::unordered_map<std::string, int> node_of_id;
    std::unordered_map<int, std::string> id_of_node;
    // (group sort key = parent id, member node ids ascending)
    std::vector<std::pair<std::string, std::vector<int>>> groups;
    std::unordered_map<uint64_t, int> weights;  // (min<<32|max) -> weight
    bool ready = false;

    // Uniform group-pair weight table: the reference's weight model
    // derives a pair's score from per-GPU facts (same devID, link type,
    // NUMA — device.go:136-158), so every partition pair of the same two
    // physical GPUs scores identically.  When that uniformity actually
    // holds in the loaded topology (verified below, not assumed), the
    // search can score candidates from per-group counts in O(G) per
    // extension instead of O(|subset|) — exact, same totals, same
    // tie-break order.  Any non-uniform pair (e.g. a partition missing a
    // link entry while its siblings have one) disables the uniform scorer.
    bool uniform = false;
    std::vector<std::vector<long>> gw;       // [group][group] pair weight
    std::unordered_map<int, int> group_of_node;

    static uint64_t pair_key(int a, int b) {
        if (a > b) std::swap(a, b);
        return ((uint64_t)(uint32_t)a << 32) | (uint32_t)b;
    }

    int weight(int a, int b) const {
        auto it = weights.find(pair_key(a, b));
        return it == weights.end() ? 0 : it->second;
    }

    void load(const std::vector<std::pair<std::string, std::vector<int>>> &groups_in,
              const std::map<std::string, int> &node_of_id_in,
              const std::vector<std::tuple<int, int, int>> &weights_in) {
        groups = groups_in;
        node_of_id.clear();
        id_of_node.clear();
        for (auto &kv : node_of_id_in) {
            node_of_id[kv.first] = kv.second;
            id_of_node[kv.second] = kv.first;
        }
        weights.clear();
        for (auto &t : weights_in)
            weights[pair_key(std::get<0>(t), std::get<1>(t))] = std::get<2>(t);
        // weights may legitimately be empty: on a no-links topology
        // (1-kfd-visible box) the policy degrades to uniform weights and
        // every pair lookup scores 0 — the search is still well-defined
        ready = !groups.empty();
        build_uniform_table();
    }

    void build_uniform_table() {
        size_t G = groups.size();
        group_of_node.clear();
        for (size_t g = 0; g < G; ++g)
            for (int n : groups[g].second) group_of_node[n] = (int)g;
        gw.assign(G, std::vector<long>(G, 0));
        uniform = true;
        for (size_t a = 0; a < G && uniform; ++a) {
            for (size_t b = a; b < G && uniform; ++b) {
                bool first = true;
                long w0 = 0;
                for (int i : groups[a].second) {
                    for (int j : groups[b].second) {
                        if (a == b && i >= j) continue;
                        long w = weight(i, j);
                        if (first) { w0 = w; first = false; }
                        else if (w != w0) { uniform = false; break; }
                    }
                    if (!uniform) break;
                }
                gw[a][b] = gw[b][a] = w0;
            }
        }
    }
};

// One request after the guards: the groups that can still contribute,
// sorted, and what is left to pick once the required nodes are set aside.
struct Request {
    const AllocState &st;
    std::vector<std::pair<std::string, std::vector<int>>> groups;  // filtered
    std::vector<int> req_nodes;
    int new_size = 0;
};

// Search state.  Every group added to an incomplete state is consumed
// FULLY (an addition only stops early when it completes the request), so
// a state is (parent set, group add order, size, weight) and its nodes
// are "the groups in add order, the last one as a prefix".  A fixed-size
// POD: no heap per state.
template <typename Extra>
struct State {
    uint64_t parents = 0;  // bitset over filtered-group indices (<=64)
    long weight = 0;
    int size = 0;
    uint8_t norder = 0;
    uint8_t order[64];     // filtered group idx, add order
    Extra x;               // the scorer's own per-state data
};

template <typename S, typename F>
void for_each_node(const Request &rq, const S &s, F fn) {
    int remaining = s.size;
    for (int oi = 0; oi < s.norder; ++oi) {
        const auto &g = rq.groups[s.order[oi]].second;
        int take = std::min((int)g.size(), remaining);
        for (int i = 0; i < take; ++i) fn(g[i]);
        remaining -= take;
    }
}

// Closed form under verified uniformity: adding m nodes of group b to a
// state with per-group counts c[] costs
//   m * sum_h c[h]*gw[b][h]  +  C(m,2)*gw[b][b]
// — O(G) per GROUP instead of O(|subset|) per NODE.
struct UniformScorer {
    struct Extra { long rowsum[64]; };  // sum_h c[h]*gw[b][h] per ORIG b
    using S = State<Extra>;
    const Request &rq;
    const size_t n_orig;
    std::vector<int> orig_of;  // filtered idx -> original group idx

    explicit UniformScorer(const Request &r)
        : rq(r), n_orig(r.st.groups.size()), orig_of(r.groups.size()) {
        // by first member node: parent keys can be ""
        for (size_t i = 0; i < rq.groups.size(); ++i)
            orig_of[i] = rq.st.group_of_node.at(rq.groups[i].second[0]);
    }
    void add_row(S &s, int b, long m) const {
        for (size_t h = 0; h < n_orig; ++h) s.x.rowsum[h] += m * rq.st.gw[b][h];
    }
    void add_group(S &s, size_t fidx, int m) const {
        int b = orig_of[fidx];
        s.weight += (long)m * s.x.rowsum[b] +
                    (long)m * (m - 1) / 2 * rq.st.gw[b][b];
        add_row(s, b, m);
    }
    void add_required(S &s) const {
        for (int rn : rq.req_nodes) {
            int b = rq.st.group_of_node.at(rn);
            s.weight += s.x.rowsum[b];
            add_row(s, b, 1);
        }
    }
};

// Exact for any weight table: each new node is scored against every node
// already in the state and the earlier new nodes of the same addition.
struct PerNodeScorer {
    struct Extra {};
    using S = State<Extra>;
    const Request &rq;
    std::vector<int> nodes;  // scratch: the state's nodes, then the new ones

    explicit PerNodeScorer(const Request &r) : rq(r) {}
    void add_node(S &s, int n) {
        for (int o : nodes) s.weight += rq.st.weight(o, n);
        nodes.push_back(n);
    }
    void add_group(S &s, size_t fidx, int m) {
        nodes.clear();
        for_each_node(rq, s, [&](int n) { nodes.push_back(n); });
        for (int i = 0; i < m; ++i) add_node(s, rq.groups[fidx].second[i]);
    }
    void add_required(S &s) {
        nodes.clear();
        for_each_node(rq, s, [&](int n) { nodes.push_back(n); });
        for (int rn : rq.req_nodes) add_node(s, rn);
    }
};

// Seed one state per group, extend breadth-first across groups, keep the
// first strict minimum among the complete states.  On success `out` holds
// the winner's nodes in generation order (seed group, then groups in add
// order, the last as a prefix), required nodes last.
template <typename Scorer>
bool search(const Request &rq, Scorer sc, std::vector<int> &out) {
    using S = typename Scorer::S;
    const size_t G = rq.groups.size();
    std::vector<S> queue;
    queue.reserve(G <= 16 ? (1u << G) : 4096);
    // parent-set dedup: direct bitmap when 2^G fits, else a set
    std::vector<bool> seen_bm;
    std::set<uint64_t> seen_set;
    const bool use_bm = G <= 20;
    if (use_bm) seen_bm.assign(1u << G, false);
    auto seen_test_set = [&](uint64_t p) {
        if (use_bm) {
            if (seen_bm[p]) return true;
            seen_bm[p] = true;
            return false;
        }
        return !seen_set.insert(p).second;
    };
    // the best final is tracked on the fly — same tie-break as collecting
    // every final and scanning, without storing them
    S best{};
    bool have_best = false;
    // add as much of group idx as the request still needs; queue the state
    // if that leaves it incomplete and its parent set is new
    auto extend = [&](S s, size_t idx) {
        int take = std::min((int)rq.groups[idx].second.size(),
                            rq.new_size - s.size);
        sc.add_group(s, idx, take);
        s.parents |= 1ull << idx;
        s.order[s.norder++] = (uint8_t)idx;
        s.size += take;
        if (s.size == rq.new_size) {
            sc.add_required(s);
            if (!have_best || s.weight < best.weight) {
                best = s;
                have_best = true;
            }
        } else if (!seen_test_set(s.parents)) {
            queue.push_back(s);
        }
    };
    for (size_t idx = 0; idx < G; ++idx) extend(S{}, idx);
    for (size_t qi = 0; qi < queue.size(); ++qi) {
        const S cur = queue[qi];
        if (__builtin_popcountll(cur.parents) == (int)G) continue;
        for (size_t idx = 0; idx < G; ++idx)
            if (!(cur.parents & (1ull << idx))) extend(cur, idx);
    }
    if (!have_best) return false;
    for_each_node(rq, best, [&](int n) { out.push_back(n); });
    out.insert(out.end(), rq.req_nodes.begin(), rq.req_nodes.end());
    return true;
}

inline bool preferred_alloc(const AllocState &st,
                            const std::vector<std::string> &available,
                            const std::vector<std::string> &required, int size,
                            std::vector<std::string> &out, std::string &err) {
    if (!st.ready) { err = "allocator not initialized"; return false; }
    if (size <= 0) { err = "allocation size must be a positive integer"; return false; }
    if ((int)available.size() < size) { err = "available devices count less than allocation size"; return false; }
    if ((int)required.size() > size) { err = "must-include set larger than allocation size"; return false; }
    if (required.size() > available.size()) { err = "must-include set larger than available set"; return false; }
    if ((int)available.size() == size) { out = available; return true; }
    if ((int)required.size() == size) { out = required; return true; }
    std::set<std::string> avail_set(available.begin(), available.end());
    for (auto &r : required)
        if (!avail_set.count(r)) { err = "must-include devices not all available"; return false; }

    Request rq{st, {}, {}, 0};
    std::set<int> avail_nodes, req_nodes;
    for (auto &a : available) {
        auto it = st.node_of_id.find(a);
        if (it != st.node_of_id.end()) avail_nodes.insert(it->second);
    }
    for (auto &r : required) {
        auto it = st.node_of_id.find(r);
        if (it != st.node_of_id.end()) {
            req_nodes.insert(it->second);
            rq.req_nodes.push_back(it->second);
        }
    }

    // filtered groups, sorted by (len asc, parent key asc)
    for (auto &g : st.groups) {
        std::vector<int> ids;
        for (int n : g.second)
            if (avail_nodes.count(n) && !req_nodes.count(n)) ids.push_back(n);
        if (!ids.empty()) rq.groups.emplace_back(g.first, std::move(ids));
    }
    // stable: Python's sort is stable, and equal (size, parent) keys must
    // tie-break identically for result parity
    std::stable_sort(rq.groups.begin(), rq.groups.end(),
                     [](auto &a, auto &b) {
                         if (a.second.size() != b.second.size())
                             return a.second.size() < b.second.size();
                         return a.first < b.first;
                     });
    if (rq.groups.size() > 64) { err = "too many device groups"; return false; }
    rq.new_size = size - (int)rq.req_nodes.size();

    // the uniform scorer's rowsum is indexed by ORIGINAL group
    const bool closed_form = st.uniform && st.groups.size() <= 64;
    std::vector<int> nodes;
    if (!(closed_form ? search(rq, UniformScorer(rq), nodes)
                      : search(rq, PerNodeScorer(rq), nodes))) {
        err = "no candidate subset found";
        return false;
    }
    for (int n : nodes) {
        auto it = st.id_of_node.find(n);
        if (it == st.id_of_node.end()) continue;
        // only the per-node path has ever re-checked the id against the
        // request; the two differ only if two ids share one node
        if (!closed_form && !avail_set.count(it->second)) continue;
        out.push_back(it->second);
    }
    return true;
}

}  // namespace prefalloc
