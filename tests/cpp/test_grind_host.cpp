// CPU check of the host-compilable merge_with_int of csrc/keccak_dev.hpp and csrc/rescue_dev.hpp (what the nonce search
// kernels run per nonce) -- the functions are __host__ __device__, so plain g++ compiles them.  One request per line on
// stdin (a letter, then five decimal 64-bit words: the seed's four digest words as a caller hands them in, and the value);
// one line of four decimal digest words per request:
//   S w0 w1 w2 w3 v   k3::merge_with_int: SHA3-256 of the 32 seed bytes followed by v as 8 little-endian bytes
//   R w0 w1 w2 w3 v   rp::merge_with_int: seed words read as BaseElement::new reads them; canonical digest words out
// tests/test_grind_host.py compares every line with hashlib and tests/rp64_util.py.
#include <stdio.h>

#include <sstream>
#include <string>

#include "../../starkpack-winterfell_amd/csrc/keccak_dev.hpp"
#include "../../starkpack-winterfell_amd/csrc/rescue_dev.hpp"

int main() {
    char buf[512];
    while (fgets(buf, sizeof(buf), stdin)) {
        std::istringstream in(buf);
        char op = 0;
        unsigned long long w[5];
        in >> op;
        for (int i = 0; i < 5; i++)
            if (!(in >> w[i])) {
                fprintf(stderr, "malformed request\n");
                return 2;
            }
        const uint64_t seed[4] = {w[0], w[1], w[2], w[3]};
        uint64_t d[4];
        if (op == 'S')
            wf::k3::merge_with_int(seed, (uint64_t)w[4], d);
        else if (op == 'R')
            wf::rp::merge_with_int(seed, (uint64_t)w[4], d);
        else {
            fprintf(stderr, "unknown request %c\n", op);
            return 2;
        }
        printf("%llu %llu %llu %llu\n", (unsigned long long)d[0], (unsigned long long)d[1], (unsigned long long)d[2], (unsigned long long)d[3]);
    }
    return 0;
}
