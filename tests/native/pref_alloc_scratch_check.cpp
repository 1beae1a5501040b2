// Stand-alone check that native/pref_alloc.h gives the same answers when
// ONE Scratch serves every request, built and run by
// tests/test_pref_alloc_scratch.py with -fsanitize=address,undefined.
//
//   pref_alloc_scratch_check CASEFILE
//
// The case file has the format of pref_alloc_check.cpp's:
//   topology NAME UNIFORM G  {PARENT N node*N}*G  I {ID node}*I  W {a b w}*W
//   case NAME SIZE  A id*A  R id*R  (ok E id*E | err)
// ("-" stands for an empty parent id).  The file's order is the test: a
// scratch that has served a large topology goes on to the smallest, and
// back.  Each case is searched on the state as loaded and on a copy with
// `uniform` forced off, through the same scratch, and then once more with a
// fresh scratch, which must agree.  Prints the number of cases checked;
// exits non-zero on the first mismatch, naming the case.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "pref_alloc.h"

namespace {

using prefalloc::AllocState;
using prefalloc::Scratch;
using Ids = std::vector<std::string>;

[[noreturn]] void die(const std::string &what) {
    std::fprintf(stderr, "pref_alloc_scratch_check: %s\n", what.c_str());
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

// the seen-sets are the one thing a request must hand on all-clear
void check_seen_clear(const std::string &name, const Scratch &sc) {
    for (uint64_t w : sc.seen_bits)
        if (w) die(name + ": seen bitmap left dirty");
    for (uint64_t w : sc.seen_hash)
        if (w) die(name + ": seen hash set left dirty");
    if (sc.seen_hash_used) die(name + ": seen hash count left non-zero");
}

// expected == nullptr: the search must fail
void check(const std::string &name, const AllocState &st, Scratch &sc,
           const Ids &available, const Ids &required, int size,
           const Ids *expected) {
    Ids out;
    std::string err;
    bool ok = prefalloc::preferred_alloc(st, sc, available, required, size,
                                         out, err);
    check_seen_clear(name, sc);
    if (!expected) {
        if (ok) die(name + ": expected an error, got" + join(out));
        if (err.empty()) die(name + ": failed without a message");
    } else {
        if (!ok) die(name + ": " + err);
        if (out != *expected)
            die(name + ": got" + join(out) + ", expected" + join(*expected));
    }
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

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) die("usage: pref_alloc_scratch_check CASEFILE");
    std::ifstream in(argv[1]);
    if (!in) die(std::string("cannot open ") + argv[1]);

    Scratch shared;  // the one scratch, for every topology and case
    AllocState st, per_node;
    std::string topology = "(none)", word;
    int cases = 0;
    while (in >> word) {
        if (word == "topology") {
            topology = read<std::string>(in);
            st = read_topology(in, topology);
            per_node = st;
            per_node.uniform = false;
        } else if (word == "case") {
            std::string name = topology + "/" + read<std::string>(in);
            int size = read<int>(in);
            Ids available = read_ids(in), required = read_ids(in);
            std::string outcome = read<std::string>(in);
            Ids expected;
            if (outcome == "ok")
                expected = read_ids(in);
            else if (outcome != "err")
                die(name + ": bad outcome '" + outcome + "'");
            const Ids *want = outcome == "ok" ? &expected : nullptr;
            check(name + " [as loaded, shared scratch]", st, shared,
                  available, required, size, want);
            check(name + " [per-node, shared scratch]", per_node, shared,
                  available, required, size, want);
            Scratch fresh;
            check(name + " [as loaded, fresh scratch]", st, fresh, available,
                  required, size, want);
            ++cases;
        } else {
            die("unexpected token '" + word + "'");
        }
    }
    std::printf("pref_alloc_scratch_check: %d cases ok\n", cases);
    return 0;
}
