/* ORACLE (test infrastructure, NOT product code): Rescue Prime over p = 2^64 - 2^32 + 1 in the plainest form that is
 * fast enough to check whole trees: canonical integers in [0, p), every product an unsigned __int128 reduced with % p,
 * both S-boxes by square-and-multiply on the bits of the exponent, the MDS product a 128-bit sum reduced with % p.
 * On purpose it shares no technique with csrc/rescue_dev.hpp or csrc/rescue_jive_dev.hpp (Montgomery residues, split
 * 32-bit accumulators, an addition chain): the one Montgomery step here turns stored residues into integers on the way
 * in (x * 2^-64 mod p).  The hasher's parameters come in at run time (rescue_ref.h); none is written down here.
 *
 *   permutation: rounds of  x^alpha | MDS | + ARK1[r] | x^inv_alpha | MDS | + ARK2[r],
 *                MDS circulant: out[i] = sum_j row[(j - i) mod w] * in[j]
 *   Rp64_256   (crypto/src/hash/rescue/rp64_256/mod.rs): state[0] = element count, elements added into the rate a block
 *                at a time, a permutation behind every full block and a partial last one; merge = hash of the 8 words
 *   RpJive64_256 (crypto/src/hash/rescue/rp64_256_jive/mod.rs): state[0] = 1 iff the count is no multiple of the rate;
 *                a partial block of i elements: rate place i SET to 1, the places behind it to 0; merge = Jive compression */
#include "rescue_ref.h"

#include <omp.h>
#include <string.h>

typedef unsigned __int128 u128;

#define P 0xFFFFFFFF00000001ull
#define MAX_W 16
#define DIGEST 4

typedef struct {
    int kind, w, rate_at, rounds;
    uint64_t alpha, inv_alpha;
    const uint64_t *row, *ark1, *ark2;
} prm_t;

static int parse(const uint64_t *b, prm_t *q) {
    if (!b) return -1;
    q->kind = (int)b[0];
    q->w = (int)b[1];
    q->rate_at = (int)b[2];
    q->rounds = (int)b[3];
    q->alpha = b[4];
    q->inv_alpha = b[5];
    if (q->kind != ORC_RESCUE_RP && q->kind != ORC_RESCUE_JIVE) return -1;
    if (q->w < 8 || q->w > MAX_W || q->rate_at != 4 || q->w - q->rate_at < DIGEST || q->rounds < 1 || q->rounds > 64) return -1;
    if (q->kind == ORC_RESCUE_JIVE && q->w != 8) return -1;
    q->row = b + 6;
    q->ark1 = q->row + q->w;
    q->ark2 = q->ark1 + (size_t)q->rounds * q->w;
    return 0;
}

static int n_threads(int threads) {
    int cap = omp_get_max_threads();
    if (cap > 16) cap = 16;
    return threads < 1 || threads > cap ? cap : threads;
}

static uint64_t mulp(uint64_t a, uint64_t b) { return (uint64_t)((u128)a * b % P); }
static uint64_t addp(uint64_t a, uint64_t b) { return (uint64_t)(((u128)a + b) % P); }

static uint64_t powp(uint64_t x, uint64_t e) {
    uint64_t r = 1;
    while (e) {
        if (e & 1) r = mulp(r, x);
        x = mulp(x, x);
        e >>= 1;
    }
    return r;
}

static void mds(const prm_t *q, uint64_t *s) {
    uint64_t o[MAX_W];
    const int w = q->w;
    for (int i = 0; i < w; i++) {
        u128 acc = 0; /* w terms below p * p / 2^57: far from 2^128 (row entries are small; each is reduced to be sure) */
        for (int j = 0; j < w; j++) acc += (u128)(q->row[(j - i + w) % w] % P) * s[j] % P;
        o[i] = (uint64_t)(acc % P);
    }
    memcpy(s, o, sizeof(uint64_t) * (size_t)w);
}

static void permute(const prm_t *q, uint64_t *s) {
    const int w = q->w;
    for (int i = 0; i < w; i++) s[i] %= P;
    for (int r = 0; r < q->rounds; r++) {
        for (int i = 0; i < w; i++) s[i] = powp(s[i], q->alpha);
        mds(q, s);
        for (int i = 0; i < w; i++) s[i] = addp(s[i], q->ark1[r * w + i] % P);
        for (int i = 0; i < w; i++) s[i] = powp(s[i], q->inv_alpha);
        mds(q, s);
        for (int i = 0; i < w; i++) s[i] = addp(s[i], q->ark2[r * w + i] % P);
    }
}

static void put_digest(const uint64_t *d, uint8_t out[32]) {
    for (int i = 0; i < DIGEST; i++)
        for (int k = 0; k < 8; k++) out[8 * i + k] = (uint8_t)(d[i] >> (8 * k));
}

static uint64_t get_word(const uint8_t *b) {
    uint64_t v = 0;
    for (int k = 0; k < 8; k++) v |= (uint64_t)b[k] << (8 * k);
    return v;
}

/* hash_elements of n canonical integers (any u64 is reduced) */
static void hash_elements(const prm_t *q, const uint64_t *e, size_t n, uint64_t d[DIGEST]) {
    uint64_t s[MAX_W] = {0};
    const size_t rate = (size_t)(q->w - q->rate_at);
    size_t i = 0;
    if (q->kind == ORC_RESCUE_RP) s[0] = (uint64_t)n % P;
    else if (n % rate) s[0] = 1;
    for (size_t k = 0; k < n; k++) {
        s[q->rate_at + i] = addp(s[q->rate_at + i], e[k] % P);
        if (++i == rate) {
            permute(q, s);
            i = 0;
        }
    }
    if (i) {
        if (q->kind == ORC_RESCUE_JIVE) {
            s[q->rate_at + i] = 1;
            for (size_t k = i + 1; k < rate; k++) s[q->rate_at + k] = 0;
        }
        permute(q, s);
    }
    memcpy(d, s + q->rate_at, sizeof(uint64_t) * DIGEST);
}

static void jive(const prm_t *q, const uint64_t init_in[8], uint64_t d[DIGEST]) {
    uint64_t init[8], fin[8];
    for (int i = 0; i < 8; i++) fin[i] = init[i] = init_in[i] % P;
    permute(q, fin);
    for (int i = 0; i < DIGEST; i++) d[i] = addp(addp(init[i], init[4 + i]), addp(fin[i], fin[4 + i]));
}

static void merge_words(const prm_t *q, const uint64_t words[8], uint64_t d[DIGEST]) {
    if (q->kind == ORC_RESCUE_RP) hash_elements(q, words, 8, d);
    else jive(q, words, d);
}

static void merge_with_int(const prm_t *q, const uint64_t seed[4], uint64_t v, uint64_t d[DIGEST]) {
    if (q->kind == ORC_RESCUE_RP) {
        uint64_t e[6] = {seed[0], seed[1], seed[2], seed[3], v % P, v / P};
        hash_elements(q, e, v >= P ? 6 : 5, d);
    } else {
        uint64_t init[8] = {seed[0], seed[1], seed[2], seed[3], v % P, 0, 0, 5};
        if (v >= P) {
            init[5] = v / P;
            init[7] = 6;
        }
        jive(q, init, d);
    }
}

int orc_rescue_permute(const uint64_t *prm, uint64_t *states, size_t n, int threads) {
    prm_t q;
    if (parse(prm, &q) || (!states && n)) return -1;
    threads = n_threads(threads);
#pragma omp parallel for num_threads(threads) schedule(static) if (n > 64)
    for (size_t i = 0; i < n; i++) permute(&q, states + i * (size_t)q.w);
    return 0;
}

int orc_rescue_hash_rows(const uint64_t *prm, const uint64_t *rows, size_t n, size_t len, size_t stride, uint8_t *digests,
                         int threads) {
    prm_t q;
    if (parse(prm, &q) || stride < len || (n && (!rows || !digests)) || len > 4096) return -1;
    const uint64_t r_inv = powp(powp(2, 64), P - 2); /* stored residue x * 2^64 -> x */
    threads = n_threads(threads);
#pragma omp parallel for num_threads(threads) schedule(static) if (n > 64)
    for (size_t i = 0; i < n; i++) {
        uint64_t e[4096], d[DIGEST];
        for (size_t k = 0; k < len; k++) e[k] = mulp(rows[i * stride + k] % P, r_inv);
        hash_elements(&q, e, len, d);
        put_digest(d, digests + 32 * i);
    }
    return 0;
}

int orc_rescue_merge(const uint64_t *prm, const uint64_t words[8], uint8_t out[32]) {
    prm_t q;
    uint64_t d[DIGEST];
    if (parse(prm, &q) || !words || !out) return -1;
    merge_words(&q, words, d);
    put_digest(d, out);
    return 0;
}

int orc_rescue_merge_with_int(const uint64_t *prm, const uint64_t seed[4], uint64_t value, uint8_t out[32]) {
    prm_t q;
    uint64_t d[DIGEST];
    if (parse(prm, &q) || !seed || !out) return -1;
    merge_with_int(&q, seed, value, d);
    put_digest(d, out);
    return 0;
}

int orc_rescue_merkle_nodes(const uint64_t *prm, const uint8_t *leaves, size_t n, uint8_t *nodes, int threads) {
    prm_t q;
    if (parse(prm, &q) || !leaves || !nodes || n < 2 || (n & (n - 1))) return -1;
    threads = n_threads(threads);
    memset(nodes, 0, 32);
    for (size_t width = n / 2; width >= 1; width /= 2) { /* the level of `width` nodes is nodes[width .. 2 width) */
#pragma omp parallel for num_threads(threads) schedule(static) if (width > 64)
        for (size_t k = width; k < 2 * width; k++) {
            const uint8_t *kids = 2 * k >= n ? leaves + 32 * (2 * k - n) : nodes + 32 * 2 * k;
            uint64_t words[8], d[DIGEST];
            for (int i = 0; i < 8; i++) words[i] = get_word(kids + 8 * i);
            merge_words(&q, words, d);
            put_digest(d, nodes + 32 * k);
        }
    }
    return 0;
}

int orc_rescue_grind(const uint64_t *prm, const uint64_t seed[4], unsigned factor, uint64_t begin, uint64_t max_nonces,
                     uint64_t *nonce, uint8_t digest[32], int threads) {
    prm_t q;
    if (parse(prm, &q) || !seed || !nonce || !digest || factor > 64) return -1;
    if (max_nonces == 0) return 0;
    const uint64_t last = begin + (max_nonces - 1) < begin ? UINT64_MAX : begin + (max_nonces - 1); /* inclusive */
    const uint64_t mask = factor == 64 ? UINT64_MAX : ((uint64_t)1 << factor) - 1;
    const uint64_t CHUNK = 256;
    const uint64_t chunks = (last - begin) / CHUNK + 1;
    threads = n_threads(threads);
    /* rounds of `threads` chunks each; a round in which some chunk found a nonce ends the search, and the answer is
     * the minimum over that round's chunks (all earlier rounds found nothing) */
    for (uint64_t c0 = 0; c0 < chunks; c0 += (uint64_t)threads) {
        uint64_t best[16];
        int have[16] = {0};
#pragma omp parallel for num_threads(threads) schedule(static, 1)
        for (int t = 0; t < threads; t++) {
            const uint64_t c = c0 + (uint64_t)t;
            if (c >= chunks) continue;
            const uint64_t lo = begin + c * CHUNK;
            const uint64_t hi = last - lo < CHUNK - 1 ? last : lo + (CHUNK - 1);
            for (uint64_t v = lo;; v++) {
                uint64_t d[DIGEST];
                merge_with_int(&q, seed, v, d);
                if ((d[0] & mask) == 0) {
                    best[t] = v;
                    have[t] = 1;
                    break;
                }
                if (v == hi) break;
            }
        }
        int any = 0;
        uint64_t min = 0;
        for (int t = 0; t < threads; t++)
            if (have[t] && (!any || best[t] < min)) {
                min = best[t];
                any = 1;
            }
        if (any) {
            uint64_t d[DIGEST];
            merge_with_int(&q, seed, min, d);
            put_digest(d, digest);
            *nonce = min;
            return 1;
        }
    }
    return 0;
}
