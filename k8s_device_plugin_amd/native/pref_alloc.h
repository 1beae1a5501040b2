// Native preferred-allocation search: the same best-effort policy as
// allocator/besteffort.py (grouping, anti-fragmentation ordering, seed +
// breadth-first extension with parent-set dedup, first strict minimum),
// written once and parametrised by how a group's nodes are scored.
//
// Everything that depends only on the allocator state is tabulated once in
// AllocState::load(): a dense node index, node->group and node->id arrays,
// the rank of every group's parent key, flat weight tables.  A request then
// works on flat arrays over those indices, and every buffer it needs lives
// in a Scratch that the caller owns and reuses, so the request path copies
// no strings and allocates nothing once the scratch has grown to size.
//
// Host-only and standard-library-only, so tests/native/pref_alloc_check.cpp
// can run it as a stand-alone program under the sanitizers; fastserver.cpp
// calls it from the GetPreferredAllocation handler.
#pragma once

#include <algorithm>
#include <cstdint>
#include <map>
#include <string>
#include <tuple>
#include <unordered_map>
#include <utility>
#include <vector>

namespace prefalloc {

struct AllocState {
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
    std::vector<long> gw;  // [group * G + group] pair weight

    // ---- tables for the request path, all derived in load() ----
    // Dense node index: position in the sorted list of every node id that
    // a group or a device id names.
    std::vector<int> node_ids;                      // dense -> node id
    std::unordered_map<std::string, int> id_index;  // device id -> id index
    std::vector<std::string> ids;                   // id index -> device id
    std::vector<int> node_of_idx;                   // id index -> dense node
    std::vector<int> id_of_dense;     // dense node -> id index, -1: none
    std::vector<int> group_of_dense;  // dense node -> group, -1: none
    std::vector<int> member_begin;    // group -> offset into members (G+1)
    std::vector<int> members;         // dense nodes, group by group
    std::vector<int> parent_rank;     // group -> rank of its parent key
    // weight by dense pair when the table is small enough to hold densely
    static constexpr size_t kDenseWeightNodes = 256;
    std::vector<int> wdense;          // [dense * N + dense], else empty

    static uint64_t pair_key(int a, int b) {
        if (a > b) std::swap(a, b);
        return ((uint64_t)(uint32_t)a << 32) | (uint32_t)b;
    }

    int weight(int a, int b) const {
        auto it = weights.find(pair_key(a, b));
        return it == weights.end() ? 0 : it->second;
    }

    int dense_weight(int a, int b) const {
        if (!wdense.empty()) return wdense[(size_t)a * node_ids.size() + b];
        return weight(node_ids[a], node_ids[b]);
    }

    int dense_of(int node) const {
        return (int)(std::lower_bound(node_ids.begin(), node_ids.end(), node) -
                     node_ids.begin());
    }

    void load(const std::vector<std::pair<std::string, std::vector<int>>> &groups_in,
              const std::map<std::string, int> &node_of_id_in,
              const std::vector<std::tuple<int, int, int>> &weights_in) {
        groups = groups_in;
        weights.clear();
        for (auto &t : weights_in)
            weights[pair_key(std::get<0>(t), std::get<1>(t))] = std::get<2>(t);
        // weights may legitimately be empty: on a no-links topology
        // (1-kfd-visible box) the policy degrades to uniform weights and
        // every pair lookup scores 0 — the search is still well-defined
        ready = !groups.empty();
        build_uniform_table();
        build_request_tables(node_of_id_in);
    }

    void build_uniform_table() {
        size_t G = groups.size();
        gw.assign(G * G, 0);
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
                gw[a * G + b] = gw[b * G + a] = w0;
            }
        }
    }

    void build_request_tables(const std::map<std::string, int> &node_of_id_in) {
        const size_t G = groups.size();
        node_ids.clear();
        for (auto &g : groups)
            node_ids.insert(node_ids.end(), g.second.begin(), g.second.end());
        for (auto &kv : node_of_id_in) node_ids.push_back(kv.second);
        std::sort(node_ids.begin(), node_ids.end());
        node_ids.erase(std::unique(node_ids.begin(), node_ids.end()),
                       node_ids.end());
        const size_t N = node_ids.size();

        // when two ids name one node, or two groups hold one node, the
        // later one (id order, group order) is the one the node maps to
        id_index.clear();
        ids.clear();
        node_of_idx.clear();
        id_of_dense.assign(N, -1);
        for (auto &kv : node_of_id_in) {
            int idx = (int)ids.size();
            id_index[kv.first] = idx;
            ids.push_back(kv.first);
            node_of_idx.push_back(dense_of(kv.second));
            id_of_dense[node_of_idx.back()] = idx;
        }
        group_of_dense.assign(N, -1);
        member_begin.assign(1, 0);
        members.clear();
        for (size_t g = 0; g < G; ++g) {
            for (int n : groups[g].second) {
                members.push_back(dense_of(n));
                group_of_dense[members.back()] = (int)g;
            }
            member_begin.push_back((int)members.size());
        }

        // equal parent keys share a rank, so comparing ranks is comparing keys
        std::vector<int> by_key(G);
        for (size_t g = 0; g < G; ++g) by_key[g] = (int)g;
        std::sort(by_key.begin(), by_key.end(), [&](int a, int b) {
            return groups[a].first < groups[b].first;
        });
        parent_rank.assign(G, 0);
        for (size_t i = 1; i < G; ++i)
            parent_rank[by_key[i]] =
                parent_rank[by_key[i - 1]] +
                (groups[by_key[i - 1]].first != groups[by_key[i]].first);

        wdense.clear();
        if (N <= kDenseWeightNodes) {
            wdense.assign(N * N, 0);
            for (size_t a = 0; a < N; ++a)
                for (size_t b = 0; b < N; ++b)
                    wdense[a * N + b] = weight(node_ids[a], node_ids[b]);
        }
    }
};

// One search state.  Every group added to an incomplete state is consumed
// FULLY (an addition only stops early when it completes the request), so
// a state is (parent set, size, weight) plus the state it was extended
// from and the group that was added: its nodes are "the groups along the
// predecessor chain in add order, the last one as a prefix".
struct SearchState {
    uint64_t parents;  // bitset over filtered-group indices (<=64)
    long weight;
    int size;
    int pred;          // index of the state this one extends; 0 is the root
    int group;         // filtered group added last
};

// Every buffer a request needs.  The caller owns it and hands the same one
// to request after request (the server keeps one, used under its mutex);
// nothing in it carries meaning from one request to the next except that
// the two seen-sets are left all-clear.
struct Scratch {
    // request: flags over id index / dense node, required nodes in order
    std::vector<uint8_t> avail_id, avail_node, req_node;
    std::vector<int> req_nodes;
    // filtered groups (those that can still contribute), sorted
    std::vector<int> fg_nodes;  // dense nodes, group by group
    struct Filtered { int begin, len, orig; };
    std::vector<Filtered> fg;
    // search: states in generation order (index 0: the empty root), the
    // uniform scorer's row sums (one row of `stride` per state), dedup
    std::vector<SearchState> states;
    std::vector<long> rows, row_tmp;
    std::vector<uint64_t> seen_bits;  // G <= 20: bitmap over parent sets
    std::vector<uint64_t> seen_hash;  // else open addressing, 0 = empty
    size_t seen_hash_used = 0;
    std::vector<int> nodes;           // per-node scorer: a state's nodes
    std::vector<int> result;          // the winner's dense nodes
};

// One request after the guards.
struct Request {
    const AllocState &st;
    Scratch &sc;
    int new_size = 0;  // what is left to pick once the required are set aside
};

// parent-set dedup: direct bitmap when 2^G bits are few, else a hash set.
// Both are cleared entry by entry from the queued states afterwards, each
// of which set exactly one entry.
struct SeenSet {
    Scratch &sc;
    const bool use_bits;

    SeenSet(Scratch &s, size_t G) : sc(s), use_bits(G <= 20) {
        if (use_bits) {
            size_t words = ((size_t(1) << G) + 63) / 64;
            if (sc.seen_bits.size() < words) sc.seen_bits.resize(words, 0);
        } else if (sc.seen_hash.empty()) {
            sc.seen_hash.assign(1024, 0);
        }
    }
    static size_t slot_of(uint64_t p, size_t mask) {
        return (size_t)((p * 0x9E3779B97F4A7C15ull) >> 20) & mask;
    }
    // true if p was already there; inserts it otherwise (p is never 0)
    bool test_set(uint64_t p) {
        if (use_bits) {
            uint64_t &w = sc.seen_bits[p >> 6], bit = 1ull << (p & 63);
            if (w & bit) return true;
            w |= bit;
            return false;
        }
        if ((sc.seen_hash_used + 1) * 2 > sc.seen_hash.size()) grow();
        size_t mask = sc.seen_hash.size() - 1;
        for (size_t i = slot_of(p, mask);; i = (i + 1) & mask) {
            if (sc.seen_hash[i] == p) return true;
            if (sc.seen_hash[i] == 0) {
                sc.seen_hash[i] = p;
                ++sc.seen_hash_used;
                return false;
            }
        }
    }
    void grow() {
        std::vector<uint64_t> old(sc.seen_hash.size() * 2, 0);
        old.swap(sc.seen_hash);
        size_t mask = sc.seen_hash.size() - 1;
        for (uint64_t p : old) {
            if (!p) continue;
            size_t i = slot_of(p, mask);
            while (sc.seen_hash[i]) i = (i + 1) & mask;
            sc.seen_hash[i] = p;
        }
    }
    void clear() {
        if (use_bits) {
            for (size_t i = 1; i < sc.states.size(); ++i)
                sc.seen_bits[sc.states[i].parents >> 6] = 0;
        } else if (sc.seen_hash_used * 8 > sc.seen_hash.size()) {
            std::fill(sc.seen_hash.begin(), sc.seen_hash.end(), 0);
            sc.seen_hash_used = 0;
        } else {
            // linear probing: an entry may sit past its home slot, so
            // empty the whole run it could be in
            size_t mask = sc.seen_hash.size() - 1;
            for (size_t s = 1; s < sc.states.size(); ++s)
                for (size_t i = slot_of(sc.states[s].parents, mask);
                     sc.seen_hash[i]; i = (i + 1) & mask)
                    sc.seen_hash[i] = 0;
            sc.seen_hash_used = 0;
        }
    }
};

// Calls fn(node) for the nodes of the state reached by adding filtered
// group `last` to state `pred`, `size` nodes in all: the groups in add
// order, the last one as a prefix.
template <typename F>
void for_each_node(const Request &rq, int pred, int last, int size, F fn) {
    int chain[65], n = 0;  // at most 64 groups, each added once
    if (last >= 0) chain[n++] = last;
    for (int s = pred; s > 0; s = rq.sc.states[s].pred)
        chain[n++] = rq.sc.states[s].group;
    int remaining = size;
    while (n-- > 0) {
        const Scratch::Filtered &g = rq.sc.fg[chain[n]];
        int take = std::min(g.len, remaining);
        for (int i = 0; i < take; ++i) fn(rq.sc.fg_nodes[g.begin + i]);
        remaining -= take;
    }
}

// A scorer prices "state `pred` plus the first `take` nodes of filtered
// group `fidx`" (add_group), then that candidate plus the required nodes
// (add_required, only for a complete candidate, right after its
// add_group), and fills in its per-state data when the candidate has been
// queued as the newest state (queued).

// Closed form under verified uniformity: adding m nodes of group b to a
// state with per-group counts c[] costs
//   m * sum_h c[h]*gw[b][h]  +  C(m,2)*gw[b][b]
// — O(G) per GROUP instead of O(|subset|) per NODE.  The row sums
// sum_h c[h]*gw[b][h], one per ORIGINAL group b, are the state's row in
// Scratch::rows.
struct UniformScorer {
    const Request &rq;
    const size_t stride;  // original groups
    const long *gw;

    explicit UniformScorer(const Request &r)
        : rq(r), stride(r.st.groups.size()), gw(r.st.gw.data()) {
        rq.sc.rows.assign(stride, 0);  // the root's row
        rq.sc.row_tmp.resize(stride);
    }
    long add_group(int pred, int fidx, int m) const {
        int b = rq.sc.fg[fidx].orig;
        return rq.sc.states[pred].weight +
               (long)m * rq.sc.rows[pred * stride + b] +
               (long)m * (m - 1) / 2 * gw[b * stride + b];
    }
    void queued(int pred, int fidx, int m) const {
        int b = rq.sc.fg[fidx].orig;
        rq.sc.rows.resize(rq.sc.states.size() * stride);
        const long *src = &rq.sc.rows[pred * stride];
        long *dst = &rq.sc.rows[(rq.sc.states.size() - 1) * stride];
        for (size_t h = 0; h < stride; ++h)
            dst[h] = src[h] + (long)m * gw[b * stride + h];
    }
    long add_required(int pred, int fidx, int m, long weight) const {
        if (rq.sc.req_nodes.empty()) return weight;
        int b = rq.sc.fg[fidx].orig;
        const long *src = &rq.sc.rows[pred * stride];
        long *row = rq.sc.row_tmp.data();
        for (size_t h = 0; h < stride; ++h)
            row[h] = src[h] + (long)m * gw[b * stride + h];
        for (int rn : rq.sc.req_nodes) {
            int rb = rq.st.group_of_dense[rn];
            if (rb < 0) continue;  // in no group: weighs nothing here
            weight += row[rb];
            for (size_t h = 0; h < stride; ++h) row[h] += gw[rb * stride + h];
        }
        return weight;
    }
};

// Exact for any weight table: each new node is scored against every node
// already in the state and the earlier new nodes of the same addition.
struct PerNodeScorer {
    const Request &rq;

    explicit PerNodeScorer(const Request &r) : rq(r) {}
    long add_node(long weight, int n) const {
        for (int o : rq.sc.nodes) weight += rq.st.dense_weight(o, n);
        rq.sc.nodes.push_back(n);
        return weight;
    }
    long add_group(int pred, int fidx, int m) const {
        rq.sc.nodes.clear();
        for_each_node(rq, pred, -1, rq.sc.states[pred].size,
                      [&](int n) { rq.sc.nodes.push_back(n); });
        long weight = rq.sc.states[pred].weight;
        const Scratch::Filtered &g = rq.sc.fg[fidx];
        for (int i = 0; i < m; ++i)
            weight = add_node(weight, rq.sc.fg_nodes[g.begin + i]);
        return weight;
    }
    void queued(int, int, int) const {}
    // Scratch::nodes still holds the candidate's nodes from add_group
    long add_required(int, int, int, long weight) const {
        for (int rn : rq.sc.req_nodes) weight = add_node(weight, rn);
        return weight;
    }
};

// Seed one state per group, extend breadth-first across groups, keep the
// first strict minimum among the complete states.  On success
// Scratch::result holds the winner's nodes in generation order (seed
// group, then groups in add order, the last as a prefix), required nodes
// last.
template <typename Scorer>
bool search(const Request &rq, const Scorer &sc) {
    Scratch &s = rq.sc;
    const size_t G = s.fg.size();
    s.states.clear();
    s.states.push_back({0, 0, 0, 0, -1});  // the empty root
    SeenSet seen(s, G);
    // the best final is tracked on the fly — same tie-break as collecting
    // every final and scanning, without storing them
    long best_weight = 0;
    int best_pred = -1, best_group = -1;
    // add as much of group idx as the request still needs; queue the state
    // if that leaves it incomplete and its parent set is new
    auto extend = [&](int pred, size_t idx) {
        const int size = s.states[pred].size;
        const int take = std::min(s.fg[idx].len, rq.new_size - size);
        long weight = sc.add_group(pred, (int)idx, take);
        const uint64_t parents = s.states[pred].parents | (1ull << idx);
        if (size + take == rq.new_size) {
            weight = sc.add_required(pred, (int)idx, take, weight);
            if (best_pred < 0 || weight < best_weight) {
                best_weight = weight;
                best_pred = pred;
                best_group = (int)idx;
            }
        } else if (!seen.test_set(parents)) {
            s.states.push_back({parents, weight, size + take, pred, (int)idx});
            sc.queued(pred, (int)idx, take);
        }
    };
    for (size_t idx = 0; idx < G; ++idx) extend(0, idx);
    for (size_t qi = 1; qi < s.states.size(); ++qi) {
        const uint64_t parents = s.states[qi].parents;
        if (__builtin_popcountll(parents) == (int)G) continue;
        for (size_t idx = 0; idx < G; ++idx)
            if (!(parents & (1ull << idx))) extend((int)qi, idx);
    }
    seen.clear();
    if (best_pred < 0) return false;
    s.result.clear();
    for_each_node(rq, best_pred, best_group, rq.new_size,
                  [&](int n) { s.result.push_back(n); });
    s.result.insert(s.result.end(), s.req_nodes.begin(), s.req_nodes.end());
    return true;
}

inline bool preferred_alloc(const AllocState &st, Scratch &sc,
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

    // duplicates and unknown ids have counted towards available.size()
    // above; only known ids reach the node set
    sc.avail_id.assign(st.ids.size(), 0);
    sc.avail_node.assign(st.node_ids.size(), 0);
    sc.req_node.assign(st.node_ids.size(), 0);
    sc.req_nodes.clear();
    for (auto &a : available) {
        auto it = st.id_index.find(a);
        if (it == st.id_index.end()) continue;
        sc.avail_id[it->second] = 1;
        sc.avail_node[st.node_of_idx[it->second]] = 1;
    }
    for (auto &r : required) {
        auto it = st.id_index.find(r);
        // an id the state does not know can still be in both lists
        if (it != st.id_index.end()
                ? !sc.avail_id[it->second]
                : std::find(available.begin(), available.end(), r) ==
                      available.end()) {
            err = "must-include devices not all available";
            return false;
        }
    }
    for (auto &r : required) {
        auto it = st.id_index.find(r);
        if (it == st.id_index.end()) continue;
        int n = st.node_of_idx[it->second];
        sc.req_node[n] = 1;
        sc.req_nodes.push_back(n);
    }

    // filtered groups, sorted by (len asc, parent key asc)
    sc.fg.clear();
    sc.fg_nodes.clear();
    for (size_t g = 0; g + 1 < st.member_begin.size(); ++g) {
        int begin = (int)sc.fg_nodes.size();
        for (int i = st.member_begin[g]; i < st.member_begin[g + 1]; ++i) {
            int n = st.members[i];
            if (sc.avail_node[n] && !sc.req_node[n]) sc.fg_nodes.push_back(n);
        }
        int len = (int)sc.fg_nodes.size() - begin;
        if (len) sc.fg.push_back({begin, len, (int)g});
    }
    if (sc.fg.size() > 64) { err = "too many device groups"; return false; }
    // stable (an insertion sort): Python's sort is stable, and equal
    // (size, parent) keys must tie-break identically for result parity
    for (size_t i = 1; i < sc.fg.size(); ++i) {
        Scratch::Filtered f = sc.fg[i];
        size_t j = i;
        for (; j > 0; --j) {
            const Scratch::Filtered &p = sc.fg[j - 1];
            bool less = f.len != p.len
                            ? f.len < p.len
                            : st.parent_rank[f.orig] < st.parent_rank[p.orig];
            if (!less) break;
            sc.fg[j] = p;
        }
        sc.fg[j] = f;
    }
    // the uniform scorer's row sums are indexed by the ORIGINAL group of a
    // filtered group's first member
    for (auto &f : sc.fg) f.orig = st.group_of_dense[sc.fg_nodes[f.begin]];

    Request rq{st, sc, size - (int)sc.req_nodes.size()};
    const bool closed_form = st.uniform && st.groups.size() <= 64;
    if (!(closed_form ? search(rq, UniformScorer(rq))
                      : search(rq, PerNodeScorer(rq)))) {
        err = "no candidate subset found";
        return false;
    }
    for (int n : sc.result) {
        int idx = st.id_of_dense[n];
        if (idx < 0) continue;
        // only the per-node path has ever re-checked the id against the
        // request; the two differ only if two ids share one node
        if (!closed_form && !sc.avail_id[idx]) continue;
        out.push_back(st.ids[idx]);
    }
    return true;
}

inline bool preferred_alloc(const AllocState &st,
                            const std::vector<std::string> &available,
                            const std::vector<std::string> &required, int size,
                            std::vector<std::string> &out, std::string &err) {
    Scratch sc;
    return preferred_alloc(st, sc, available, required, size, out, err);
}

}  // namespace prefalloc
