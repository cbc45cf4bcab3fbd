// CPU check of csrc/rescue_dev.hpp (the Rp64_256 the device kernels run) -- the functions are __host__ __device__, so plain
// g++ compiles them.  Reads one request per line from stdin (a letter, then decimal 64-bit words) and prints one line of
// decimal words per request:
//   P w0 .. w11   the permutation, one lane per permutation (permute): canonical state in, canonical state out
//   Q w0 .. w11   the same through the lane form's host code (permute_lanes_host: per-lane S-boxes and MDS rows)
//   H e0 .. en-1  hash_elements of n canonical elements (n may be 0 .. any) -> the 4 canonical digest words
//   M w0 .. w7    merge of two digests; the words are taken as a caller hands them in (any u64, reduced as BaseElement::new)
//   L w0 .. w7    merge through the lane form's start values (merge_lane_init) and permute_lanes_host
//   T             the tables as the header holds them: 84 ARK1 words, 84 ARK2 words (Montgomery form), 12 MDS entries
// tests/test_rescue_host.py compares every line with tests/rp64_util.py (Python integers).
#include <stdio.h>
#include <stdlib.h>

#include <sstream>
#include <string>
#include <vector>

#include "../../starkpack-winterfell_amd/csrc/rescue_dev.hpp"

using wf::F64;
namespace rp = wf::rp;

static void print_words(const uint64_t *w, size_t n) {
    for (size_t i = 0; i < n; i++) printf(i ? " %llu" : "%llu", (unsigned long long)w[i]);
    printf("\n");
}

int main() {
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
            if (w.size() != 12) {
                fprintf(stderr, "%c needs 12 words\n", op);
                return 2;
            }
            uint64_t s[12];
            for (int i = 0; i < 12; i++) s[i] = rp::elem_new(w[i]);
            if (op == 'P') rp::permute(s);
            else rp::permute_lanes_host(s);
            for (int i = 0; i < 12; i++) s[i] = F64::to_canonical(s[i]);
            print_words(s, 12);
        } else if (op == 'H') {
            size_t at = 0;
            uint64_t d[4];
            rp::hash_elements(w.size(), [&]() { return rp::elem_new(w[at++]); }, d);
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
            uint64_t d[4];
            if (op == 'M') {
                uint64_t m[8];
                for (int i = 0; i < 8; i++) m[i] = w[i];
                rp::merge(m, d);
            } else {
                uint64_t s[12];
                for (uint32_t i = 0; i < 12; i++) s[i] = rp::merge_lane_init(i, i >= 4 ? w[i - 4] : 0);
                rp::permute_lanes_host(s);
                for (int i = 0; i < 4; i++) d[i] = F64::to_canonical(s[4 + i]);
            }
            print_words(d, 4);
        } else if (op == 'T') {
            std::vector<uint64_t> t;
            for (int half = 0; half < 2; half++)
                for (int r = 0; r < rp::ROUNDS; r++)
                    for (uint32_t i = 0; i < 12; i++) t.push_back(rp::ark(half, r, i));
            for (int k = 0; k < 12; k++) t.push_back(rp::mds_coef(k));
            print_words(t.data(), t.size());
        } else {
            fprintf(stderr, "unknown request %c\n", op);
            return 2;
        }
    }
    return 0;
}
