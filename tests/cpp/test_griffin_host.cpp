// CPU check of csrc/griffin_dev.hpp (the GriffinJive64_256 the device kernels run) -- the functions are __host__ __device__,
// so plain g++ compiles them.  Reads one request per line from stdin (a letter, then decimal 64-bit words) and prints one
// line of decimal words per request:
//   P w0 .. w7     the permutation (permute): canonical state in, canonical state out
//   N w0 .. w7     the non-linear layer alone (nonlinear): canonical in, canonical out
//   H e0 .. en-1   hash_elements of n canonical elements (n may be 0 .. any) -> the 4 canonical digest words
//   M w0 .. w7     merge of two digests; the words are taken as a caller hands them in (any u64, reduced as BaseElement::new)
//   I s0 .. s3 v   merge_with_int of the seed words (any u64) and the 64-bit value v
//   D i z0 z1 t    linear(i, z0, z1, t) on raw residues below p (i = 2..7) -> one raw residue.  linear_uncorrected below is
//                  a copy of linear without its last correction.  Once a D request was seen, the program FAILS (exit 4)
//                  unless, for every i = 2..7, some D request told the copy from the real function -- as
//                  test_rpjive_host.cpp does for the plain-+ copy of mds_row.
//   T              the tables as the header holds them (Montgomery form): 48 ARK words, 6 ALPHA, 6 BETA, then the 8 MDS entries
//   K              MERKLE_PLAN_GRIFFIN through merkle_next_launch for n_leaves = 2^1 .. 2^34, the tuning values and the CU
//                  counts of test_merkle_plan.cpp: prints <sequences checked> <violations>
// tests/test_griffin_host.py compares every line with tests/griffin_util.py (Python integers) and tests/cpp/griffin_ref.c.
#include <stdio.h>
#include <stdlib.h>

#include <sstream>
#include <string>
#include <vector>

#include "../../starkpack-winterfell_amd/csrc/griffin_dev.hpp"
#include "../../starkpack-winterfell_amd/csrc/merkle_plan.hpp"

using wf::F64;
namespace rp = wf::rp;
namespace rpj = wf::rpj;
namespace gfj = wf::gfj;

static void print_words(const uint64_t *w, size_t n) {
    for (size_t i = 0; i < n; i++) printf(i ? " %llu" : "%llu", (unsigned long long)w[i]);
    printf("\n");
}

// The levels of every launch sum to log2 n, children halve level by level down to one node, every grid is below 2^31, a
// sub-tree launch has the kernel's work-group size, spans one parent per lane and folds no more levels than that span holds,
// and the wide kernel is only asked for levels of at least 2^level_min_log parents.
static void check_plan() {
    const wf::MerklePlan &plan = wf::MERKLE_PLAN_GRIFFIN;
    const uint32_t cus[] = {1, 64, 256, 304};
    uint64_t checked = 0, bad = 0;
    for (uint32_t log_n = 1; log_n <= 34; log_n++) {
        for (uint32_t l2_min = 10; l2_min <= 30; l2_min += 5) {
            for (uint32_t num_cus : cus) {
                uint64_t n_children = (uint64_t)1 << log_n;
                uint32_t levels = 0, steps = 0;
                bool ok = true;
                while (n_children > 1 && steps < 64) {
                    const wf::MerkleStep s = wf::merkle_next_launch(n_children, plan, l2_min, num_cus);
                    const uint64_t n_par = n_children >> 1;
                    ok = ok && s.levels >= 1 && s.n_children == n_children >> s.levels && s.grid >= 1 && s.grid < ((uint64_t)1 << 31);
                    if (s.kind == wf::MERKLE_SUBTREE) {
                        // k_merkle_subtree<M>: one lane per parent of the first level, 256 lanes (its LDS array and launch bounds)
                        ok = ok && s.block == plan.subtree_threads && s.block == 256 && plan.subtree_span == 256;
                        ok = ok && s.levels <= plan.subtree_levels && ((uint64_t)plan.subtree_span >> (s.levels - 1)) >= 1;
                        ok = ok && s.grid * plan.subtree_span >= n_par && (s.grid - 1) * plan.subtree_span < n_par;
                        ok = ok && n_par < ((uint64_t)1 << plan.level_min_log);
                        if (s.grid > 1) ok = ok && n_par % plan.subtree_span == 0;  // every work-group starts full
                    } else {
                        ok = ok && s.kind == wf::MERKLE_LEVEL && s.levels == 1 && s.block == 256 && s.grid * 256 >= n_par;
                        ok = ok && n_par >= ((uint64_t)1 << plan.level_min_log);
                    }
                    levels += s.levels;
                    n_children = s.n_children;
                    steps++;
                }
                ok = ok && n_children == 1 && levels == log_n;
                checked++;
                bad += ok ? 0 : 1;
            }
        }
    }
    const uint64_t out[2] = {checked, bad};
    print_words(out, 2);
}

// gfj::linear without its last correction: the folded sum as the 64-bit adder leaves it.
static uint64_t linear_uncorrected(int i, uint64_t z0, uint64_t z1, uint64_t t) {
    const uint64_t k = (uint64_t)(i - 1);
    const uint64_t lo = k * (uint32_t)z0 + (uint32_t)z1 + (uint32_t)t;
    const uint64_t hi = k * (uint32_t)(z0 >> 32) + (uint32_t)(z1 >> 32) + (uint32_t)(t >> 32);
    const uint64_t s_lo = lo + (hi << 32);
    const uint64_t s_hi = (hi >> 32) + (s_lo < lo ? 1u : 0u);
    return s_lo + ((s_hi << 32) - s_hi);
}

static bool need(const std::vector<uint64_t> &w, size_t n, char op) {
    if (w.size() == n) return true;
    fprintf(stderr, "%c needs %zu words\n", op, n);
    return false;
}

int main() {
    bool directed_seen = false, told_apart[8] = {};
    std::string line;
    std::vector<std::string> lines;
    int c;
    while ((c = getchar()) != EOF) {
        if (c == '\n') {
            lines.push_back(line);
            line.clear();
        } else {
            line.push_back((char)c);
        }
    }
    if (!line.empty()) lines.push_back(line);
    for (const std::string &l : lines) {
        std::istringstream in(l);
        char op = 0;
        in >> op;
        std::vector<uint64_t> w;
        unsigned long long v;
        while (in >> v) w.push_back((uint64_t)v);
        if (!in.eof()) {
            fprintf(stderr, "malformed request\n");
            return 2;
        }
        if (op == 'P' || op == 'N') {
            if (!need(w, 8, op)) return 2;
            uint64_t s[8];
            for (int i = 0; i < 8; i++) s[i] = rp::elem_new(w[i]);
            if (op == 'P') gfj::permute(s);
            else gfj::nonlinear(s);
            for (int i = 0; i < 8; i++) s[i] = F64::to_canonical(s[i]);
            print_words(s, 8);
        } else if (op == 'H') {
            size_t at = 0;
            uint64_t d[4];
            gfj::hash_elements(w.size(), [&]() { return rp::elem_new(w[at++]); }, d);
            if (at != w.size()) {
                fprintf(stderr, "absorber pulled %zu elements of %zu\n", at, w.size());
                return 3;
            }
            print_words(d, 4);
        } else if (op == 'M') {
            if (!need(w, 8, op)) return 2;
            uint64_t m[8], d[4];
            for (int i = 0; i < 8; i++) m[i] = w[i];
            gfj::merge(m, d);
            print_words(d, 4);
        } else if (op == 'I') {
            if (!need(w, 5, op)) return 2;
            uint64_t s[4], d[4];
            for (int i = 0; i < 4; i++) s[i] = w[i];
            gfj::merge_with_int(s, w[4], d);
            print_words(d, 4);
        } else if (op == 'D') {
            if (!need(w, 4, op)) return 2;
            if (w[0] < 2 || w[0] > 7 || w[1] >= F64::P || w[2] >= F64::P || w[3] >= F64::P) {
                fprintf(stderr, "D takes i = 2..7 and raw residues below p\n");
                return 2;
            }
            const int i = (int)w[0];
            const uint64_t got = gfj::linear(i, w[1], w[2], w[3]);
            directed_seen = true;
            if (linear_uncorrected(i, w[1], w[2], w[3]) != got) told_apart[i] = true;
            print_words(&got, 1);
        } else if (op == 'T') {
            std::vector<uint64_t> t;
            for (int r = 0; r < gfj::ROUNDS - 1; r++)
                for (uint32_t i = 0; i < 8; i++) t.push_back(gfj::ark(r, i));
            for (int i = 0; i < 6; i++) t.push_back(gfj::alpha(i));
            for (int i = 0; i < 6; i++) t.push_back(gfj::beta(i));
            for (int k = 0; k < 8; k++) t.push_back(rpj::mds_coef(k));
            print_words(t.data(), t.size());
        } else if (op == 'K') {
            check_plan();
        } else {
            fprintf(stderr, "unknown request %c\n", op);
            return 2;
        }
    }
    if (directed_seen) {
        for (int i = 2; i < 8; i++) {
            if (!told_apart[i]) {
                fprintf(stderr, "no directed operand told linear from its uncorrected copy for i = %d\n", i);
                return 4;
            }
        }
    }
    return 0;
}
