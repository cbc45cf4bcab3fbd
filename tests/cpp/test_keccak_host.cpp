// CPU check of csrc/keccak_dev.hpp (the SHA3-256 the device kernels run) -- the functions are __host__ __device__, so plain
// g++ compiles them.  Reads one request per line from stdin and prints one digest (hex) per line:
//   B <hex>   SHA3-256 of the bytes, any length (sha3_256_bytes)
//   L <hex>   the same through the lane-granular absorber the kernels use (length a multiple of 8)
//   M <hex>   merge of two digests (64 bytes)
// tests/test_keccak_host.py compares every line with hashlib.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../starkpack-winterfell_amd/csrc/keccak_dev.hpp"

static int nibble(int c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    return -1;
}

static uint64_t lane_at(const std::vector<unsigned char> &m, size_t i) {
    uint64_t w = 0;
    for (int b = 7; b >= 0; b--) w = (w << 8) | m[8 * i + b];
    return w;
}

static void print_lanes(const uint64_t (&d)[4]) {
    for (int i = 0; i < 4; i++)
        for (int b = 0; b < 8; b++) printf("%02x", (unsigned)((d[i] >> (8 * b)) & 0xff));
    printf("\n");
}

int main() {
    std::string line;
    int c;
    std::vector<std::string> lines;
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
        if (l.size() < 2 || l[1] != ' ' || (l.size() - 2) % 2) {
            fprintf(stderr, "malformed request\n");
            return 2;
        }
        std::vector<unsigned char> msg((l.size() - 2) / 2);
        for (size_t i = 0; i < msg.size(); i++) {
            const int hi = nibble(l[2 + 2 * i]), lo = nibble(l[3 + 2 * i]);
            if (hi < 0 || lo < 0) {
                fprintf(stderr, "malformed hex\n");
                return 2;
            }
            msg[i] = (unsigned char)(hi * 16 + lo);
        }
        if (l[0] == 'B') {
            unsigned char d[32];
            wf::k3::sha3_256_bytes(msg.data(), msg.size(), d);
            for (int i = 0; i < 32; i++) printf("%02x", d[i]);
            printf("\n");
        } else if (l[0] == 'L') {
            if (msg.size() % 8) {
                fprintf(stderr, "L needs whole lanes\n");
                return 2;
            }
            size_t at = 0;
            uint64_t d[4];
            wf::k3::sha3_256_lanes(msg.size() / 8, [&]() { return lane_at(msg, at++); }, d);
            if (at != msg.size() / 8) {
                fprintf(stderr, "absorber pulled %zu lanes of %zu\n", at, msg.size() / 8);
                return 3;
            }
            print_lanes(d);
        } else if (l[0] == 'M') {
            if (msg.size() != 64) {
                fprintf(stderr, "M needs 64 bytes\n");
                return 2;
            }
            uint64_t in[8], d[4];
            for (int i = 0; i < 8; i++) in[i] = lane_at(msg, i);
            wf::k3::sha3_merge(in, d);
            print_lanes(d);
        } else {
            fprintf(stderr, "unknown request %c\n", l[0]);
            return 2;
        }
    }
    return 0;
}
