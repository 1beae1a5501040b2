// Stand-alone check of native/pref_alloc.h, built and run by
// tests/test_pref_alloc_native.py with -fsanitize=address,undefined.
//
//   pref_alloc_check CASEFILE
//
// The case file is whitespace-separated tokens ("-" stands for an empty
// parent id):
//   topology NAME UNIFORM G  {PARENT N node*N}*G  I {ID node}*I  W {a b w}*W
//   case NAME SIZE  A id*A  R id*R  (ok E id*E | err)
// A case belongs to the topology before it.  Each is searched twice — on
// the state as loaded and on a copy with `uniform` forced off, which
// selects the per-node scorer — and both must give the expected id list,
// or both fail where an error is expected.  Prints the number of cases
// checked; exits non-zero on the first mismatch, naming the case.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <set>
#include <string>
#include <vector>

#include "pref_alloc.h"

namespace {

using prefalloc::AllocState;
using Ids = std::vector<std::string>;

[[noreturn]] void die(const std::string &what) {
    std::fprintf(stderr, "pref_alloc_check: %s\n", what.c_str());
    std::exit(1);
}

template <typename T>
T read(std::istream &in) {
    T v;
    if (!(in >> v)) die("truncated case file");
    return v;
}

Ids read_ids(std::istream &in) {
    Ids ids(read<size_t>(in));
    for (auto &id : ids) id = read<std::string>(in);
    return ids;
}

std::string join(const Ids &ids) {
    std::string s;
    for (auto &id : ids) s += " " + id;
    return s;
}

// expected == nullptr: the search must fail
void check(const std::string &name, const AllocState &st, const char *scorer,
           const Ids &available, const Ids &required, int size,
           const Ids *expected) {
    Ids out;
    std::string err;
    bool ok = prefalloc::preferred_alloc(st, available, required, size, out, err);
    if (!expected) {
        if (ok) die(name + " [" + scorer + "]: expected an error, got" + join(out));
        if (err.empty()) die(name + " [" + scorer + "]: failed without a message");
    } else {
        if (!ok) die(name + " [" + scorer + "]: " + err);
        if (out != *expected)
            die(name + " [" + scorer + "]: got" + join(out) + ", expected" +
                join(*expected));
    }
}

void check_both(const std::string &name, const AllocState &st,
                const Ids &available, const Ids &required, int size,
                const Ids *expected) {
    AllocState per_node = st;
    per_node.uniform = false;
    check(name, st, "as loaded", available, required, size, expected);
    check(name, per_node, "per-node", available, required, size, expected);
}

AllocState read_topology(std::istream &in, const std::string &name) {
    bool uniform = read<int>(in) != 0;
    std::vector<std::pair<std::string, std::vector<int>>> groups(read<size_t>(in));
    for (auto &g : groups) {
        g.first = read<std::string>(in);
        if (g.first == "-") g.first.clear();
        g.second.resize(read<size_t>(in));
        for (int &n : g.second) n = read<int>(in);
    }
    std::map<std::string, int> node_of_id;
    for (size_t i = read<size_t>(in); i > 0; --i) {
        std::string id = read<std::string>(in);
        node_of_id[id] = read<int>(in);
    }
    std::vector<std::tuple<int, int, int>> weights(read<size_t>(in));
    for (auto &w : weights) {
        int a = read<int>(in), b = read<int>(in);
        w = std::make_tuple(a, b, read<int>(in));
    }
    AllocState st;
    st.load(groups, node_of_id, weights);
    if (!st.ready) die(name + ": not ready after load");
    if (st.uniform != uniform)
        die(name + ": uniform is " + std::to_string(st.uniform) +
            " after load, the file records " + std::to_string(uniform));
    return st;
}

// More original groups than the uniform scorer's table holds, and more
// filtered groups than the parent bitset holds.
void check_65_groups() {
    std::vector<std::pair<std::string, std::vector<int>>> groups;
    std::map<std::string, int> node_of_id;
    Ids all;
    for (int i = 0; i < 65; ++i) {
        std::string id = "dev" + std::to_string(100 + i);
        groups.push_back({id, {i + 1}});
        node_of_id[id] = i + 1;
        all.push_back(id);
    }
    AllocState st;
    st.load(groups, node_of_id, {});
    if (!st.ready) die("65 groups: not ready after load");

    for (bool uniform : {st.uniform, false}) {
        AllocState s = st;
        s.uniform = uniform;
        Ids out;
        std::string err;
        if (prefalloc::preferred_alloc(s, all, {}, 2, out, err) ||
            err != "too many device groups")
            die("65 groups, all available: expected 'too many device groups', got '" +
                err + "'");
        Ids ten(all.begin() + 20, all.begin() + 30);
        out.clear();
        if (!prefalloc::preferred_alloc(s, ten, {}, 2, out, err))
            die("65 groups, 10 available: " + err);
        std::set<std::string> avail(ten.begin(), ten.end());
        if (out.size() != 2 || out[0] == out[1] || !avail.count(out[0]) ||
            !avail.count(out[1]))
            die("65 groups, 10 available: got" + join(out));
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) die("usage: pref_alloc_check CASEFILE");
    std::ifstream in(argv[1]);
    if (!in) die(std::string("cannot open ") + argv[1]);

    AllocState st;
    std::string topology = "(none)", word;
    int cases = 0;
    while (in >> word) {
        if (word == "topology") {
            topology = read<std::string>(in);
            st = read_topology(in, topology);
        } else if (word == "case") {
            std::string name = topology + "/" + read<std::string>(in);
            int size = read<int>(in);
            Ids available = read_ids(in), required = read_ids(in);
            std::string outcome = read<std::string>(in);
            if (outcome == "ok") {
                Ids expected = read_ids(in);
                check_both(name, st, available, required, size, &expected);
            } else if (outcome == "err") {
                check_both(name, st, available, required, size, nullptr);
            } else {
                die(name + ": bad outcome '" + outcome + "'");
            }
            ++cases;
        } else {
            die("unexpected token '" + word + "'");
        }
    }
    check_65_groups();
    std::printf("pref_alloc_check: %d cases ok\n", cases);
    return 0;
}
