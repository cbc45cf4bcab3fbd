// CPU check of csrc/rescue_jive_dev.hpp (the RpJive64_256 the device kernels run) -- the functions are __host__ __device__,
// so plain g++ compiles them.  Reads one request per line from stdin (a letter, then decimal 64-bit words) and prints one
// line of decimal words per request:
//   P w0 .. w7     the permutation, one lane per permutation (permute): canonical state in, canonical state out
//   Q w0 .. w7     the same through the lane form's host code (permute_lanes_host: per-lane S-boxes and MDS rows)
//   H e0 .. en-1   hash_elements of n canonical elements (n may be 0 .. any) -> the 4 canonical digest words
//   M w0 .. w7     merge of two digests; the words are taken as a caller hands them in (any u64, reduced as BaseElement::new)
//   L w0 .. w7     merge through the lane form's host code (merge_lanes_host: t = init + fin per lane, lanes 0..3 add lane + 4)
//   I s0 .. s3 v   merge_with_int of the seed words (any u64) and the 64-bit value v
//   D i f y0 .. y7 the linear layer alone on a state of raw residues (what stands behind the first S-box): 8 words of mds_ark
//                  (one-lane form) then 8 of lane_mds_ark (lane form), both with ARK1 of round 0, as raw residues.  f = 1
//                  marks a state built so that the closing addition of row i wraps (tests/rescue_edge_util.py, case 1):
//                  mds_row_plain_plus below, a copy of mds_row that ends in a plain +, must differ from mds_row there.
//                  Once a D request was seen, the program FAILS (exit 4) unless such states told the copy from the real
//                  function on every row -- as test_field_edges.cpp does for the wrong-mask reduction.
//   T              the tables as the header holds them: 56 ARK1 words, 56 ARK2 words (Montgomery form), 8 MDS entries
//   K              MERKLE_PLAN_RPJIVE through merkle_next_launch for n_leaves = 2^1 .. 2^34 and the CU counts of
//                  test_merkle_plan.cpp: prints <sequences checked> <violations>
// tests/test_rpjive_host.py compares every line with tests/rpjive_util.py (Python integers).
#include <stdio.h>
#include <stdlib.h>

#include <sstream>
#include <string>
#include <vector>

#include "../../starkpack-winterfell_amd/csrc/merkle_plan.hpp"
#include "../../starkpack-winterfell_amd/csrc/rescue_jive_dev.hpp"

using wf::F64;
namespace rp = wf::rp;
namespace rpj = wf::rpj;

static void print_words(const uint64_t *w, size_t n) {
    for (size_t i = 0; i < n; i++) printf(i ? " %llu" : "%llu", (unsigned long long)w[i]);
    printf("\n");
}

// The levels of every launch sum to log2 n, the sequence ends at one node, every grid is below 2^31, a sub-tree launch has
// the kernel's work-group size and never more levels than its span folds, and the wide kernel is only asked for levels of at
// least 2^level_min_log parents.
static void check_plan() {
    const wf::MerklePlan &plan = wf::MERKLE_PLAN_RPJIVE;
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
                        ok = ok && s.block == plan.subtree_threads && s.block == 8 * plan.subtree_span && s.levels <= plan.subtree_levels;
                        ok = ok && s.grid * plan.subtree_span >= n_par && (s.grid - 1) * plan.subtree_span < n_par;
                        ok = ok && n_par < ((uint64_t)1 << plan.level_min_log);
                        // more than one work-group: every one of them starts full, and folds no further than to one node
                        if (s.grid > 1) ok = ok && n_par % plan.subtree_span == 0 && (plan.subtree_span >> (s.levels - 1)) >= 1;
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

// rpj::mds_row with its closing canonical addition replaced by a plain 64-bit +: the mistake the directed states exist for.
template <class Get>
static uint64_t mds_row_plain_plus(uint32_t i, Get &&get) {
    uint64_t lo = 0, hi = 0;
    for (int k = 0; k < rpj::STATE; k++) {
        uint32_t j = i + (uint32_t)k;
        j -= j >= (uint32_t)rpj::STATE ? (uint32_t)rpj::STATE : 0u;
        const uint64_t v = get(j);
        lo += (uint64_t)rpj::mds_coef(k) * (uint32_t)v;
        hi += (uint64_t)rpj::mds_coef(k) * (uint32_t)(v >> 32);
    }
    const uint64_t top = hi >> 32;
    return (hi << 32) + (lo + ((top << 32) - top));
}

int main() {
    bool directed_seen = false, told_apart[rpj::STATE] = {};
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
        if (op == 'P' || op == 'Q') {
            if (w.size() != 8) {
                fprintf(stderr, "%c needs 8 words\n", op);
                return 2;
            }
            uint64_t s[8];
            for (int i = 0; i < 8; i++) s[i] = rp::elem_new(w[i]);
            if (op == 'P') rpj::permute(s);
            else rpj::permute_lanes_host(s);
            for (int i = 0; i < 8; i++) s[i] = F64::to_canonical(s[i]);
            print_words(s, 8);
        } else if (op == 'H') {
            size_t at = 0;
            uint64_t d[4];
            rpj::hash_elements(w.size(), [&]() { return rp::elem_new(w[at++]); }, d);
            if (at != w.size()) {
                fprintf(stderr, "absorber pulled %zu elements of %zu\n", at, w.size());
                return 3;
            }
            print_words(d, 4);
        } else if (op == 'M' || op == 'L') {
            if (w.size() != 8) {
                fprintf(stderr, "%c needs 8 words\n", op);
                return 2;
            }
            uint64_t m[8], d[4];
            for (int i = 0; i < 8; i++) m[i] = w[i];
            if (op == 'M') rpj::merge(m, d);
            else rpj::merge_lanes_host(m, d);
            print_words(d, 4);
        } else if (op == 'I') {
            if (w.size() != 5) {
                fprintf(stderr, "I needs 5 words\n");
                return 2;
            }
            uint64_t s[4], d[4];
            for (int i = 0; i < 4; i++) s[i] = w[i];
            rpj::merge_with_int(s, w[4], d);
            print_words(d, 4);
        } else if (op == 'D') {
            constexpr int W = rpj::STATE;
            if (w.size() != 2 + (size_t)W || w[0] >= (uint64_t)W || w[1] > 1) {
                fprintf(stderr, "D needs a row, a flag and %d words\n", W);
                return 2;
            }
            uint64_t s[W], m[W], o[2 * W];
            for (int i = 0; i < W; i++) {
                s[i] = w[2 + i];
                if (s[i] >= F64::P) {
                    fprintf(stderr, "D takes raw residues below p\n");
                    return 2;
                }
            }
            auto get = [&](uint32_t j) { return s[j]; };
            for (int i = 0; i < W; i++) m[i] = s[i];
            rpj::mds_ark(m, 0, 0);
            for (int i = 0; i < W; i++) o[i] = m[i];
            for (int i = 0; i < W; i++) o[W + i] = rpj::lane_mds_ark((uint32_t)i, 0, 0, get);
            directed_seen = true;
            const uint32_t row = (uint32_t)w[0];
            if (w[1] && mds_row_plain_plus(row, get) != rpj::mds_row(row, get)) told_apart[row] = true;
            print_words(o, 2 * W);
        } else if (op == 'T') {
            std::vector<uint64_t> t;
            for (int half = 0; half < 2; half++)
                for (int r = 0; r < rpj::ROUNDS; r++)
                    for (uint32_t i = 0; i < 8; i++) t.push_back(rpj::ark(half, r, i));
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
        for (int i = 0; i < rpj::STATE; i++) {
            if (!told_apart[i]) {
                fprintf(stderr, "no case-1 state told mds_row from its plain-+ copy on row %d\n", i);
                return 4;
            }
        }
    }
    return 0;
}
