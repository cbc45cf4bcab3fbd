/* A plain C reference of GriffinJive64_256 for the tests (tests/griffin_util.py builds it with `cc -O2 -shared -fPIC` and
 * loads it with ctypes; tests/test_griffin_host.py pins it to the Python-integer restatement).  Deliberately unlike
 * csrc/griffin_dev.hpp: canonical integers throughout, unsigned __int128 products reduced with %, both S-boxes by
 * square-and-multiply on the exponent's bits, the MDS product as a 128-bit sum -- no Montgomery form, no addition chain, no
 * folded reductions.  The parameters are read from tests/golden/griffinjive64_256_params.json at run time (gfr_load).
 *
 *   state: 8 elements, rate 0..4, capacity 4..8, digest 0..4
 *   permutation: 7 rounds of non-linear | MDS | + ARK[r], no constants behind the last round
 *   rows handed to gfr_hash_rows are STORED elements (x * 2^64 mod p, as the library takes them): made canonical first
 *   digests are 4 canonical little-endian u64; digest words read are reduced mod p
 * Rows and tree levels are split over up to 8 threads. */
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef unsigned __int128 u128;
#define W 8
#define ROUNDS 7
static const uint64_t P = 0xFFFFFFFF00000001ull;
#define MAX_THREADS 8

static struct {
    int loaded;
    uint64_t alpha, inv_alpha, row[W], ark[ROUNDS - 1][W], alpha_i[W - 2], beta_i[W - 2], r_inv;
} G;

/* the numbers behind "key" in the JSON text: one number, or every number of the (nested) array that follows */
static int numbers_of(const char *text, const char *key, uint64_t *out, int want) {
    char pat[64];
    snprintf(pat, sizeof pat, "\"%s\"", key);
    const char *p = strstr(text, pat);
    if (!p) return -1;
    p = strchr(p + strlen(pat), ':');
    if (!p) return -1;
    p++;
    int depth = 0, n = 0;
    for (;; p++) {
        if (*p == 0) return -1;
        if (*p == '[') depth++;
        else if (*p == ']') {
            if (--depth <= 0) break;
        } else if (*p >= '0' && *p <= '9') {
            char *end;
            const unsigned long long v = strtoull(p, &end, 10);
            if (n < want) out[n] = (uint64_t)v;
            n++;
            p = end - 1;
            if (depth == 0) break;
        } else if (depth == 0 && (*p == ',' || *p == '}')) break;
    }
    return n == want ? 0 : -2;
}

static uint64_t mulp(uint64_t a, uint64_t b) { return (uint64_t)((u128)a * b % P); }
static uint64_t addp(uint64_t a, uint64_t b) { return (uint64_t)(((u128)a + b) % P); }
static uint64_t powp(uint64_t x, uint64_t e) {
    uint64_t r = 1;
    for (int bit = 63; bit >= 0; bit--) {
        r = mulp(r, r);
        if ((e >> bit) & 1) r = mulp(r, x);
    }
    return r;
}

int gfr_load(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) return 1;
    static char text[1 << 16];
    const size_t n = fread(text, 1, sizeof text - 1, f);
    fclose(f);
    text[n] = 0;
    uint64_t one[1];
    if (numbers_of(text, "modulus", one, 1) || one[0] != P) return 2;
    if (numbers_of(text, "state_width", one, 1) || one[0] != W) return 3;
    if (numbers_of(text, "num_rounds", one, 1) || one[0] != ROUNDS) return 4;
    if (numbers_of(text, "alpha", &G.alpha, 1)) return 5;
    if (numbers_of(text, "inv_alpha", &G.inv_alpha, 1)) return 6;
    if (numbers_of(text, "mds_row", G.row, W)) return 7;
    if (numbers_of(text, "ark", &G.ark[0][0], (ROUNDS - 1) * W)) return 8;
    if (numbers_of(text, "alpha_i", G.alpha_i, W - 2)) return 9;
    if (numbers_of(text, "beta_i", G.beta_i, W - 2)) return 10;
    G.r_inv = powp((uint64_t)(((u128)1 << 64) % P), P - 2); /* 2^-64 mod p: stored -> canonical */
    G.loaded = 1;
    return 0;
}

static void nonlinear(uint64_t *s) {
    s[0] = powp(s[0], G.inv_alpha);
    s[1] = powp(s[1], G.alpha);
    for (int i = 2; i < W; i++) {
        const u128 sum = (u128)(i - 1) * s[0] + s[1] + (i > 2 ? s[i - 1] : 0);
        const uint64_t l = (uint64_t)(sum % P);
        const uint64_t q = addp(addp(mulp(l, l), mulp(G.alpha_i[i - 2], l)), G.beta_i[i - 2]);
        s[i] = mulp(s[i], q);
    }
}

static void mds(uint64_t *s) {
    uint64_t o[W];
    for (int i = 0; i < W; i++) {
        u128 acc = 0;
        for (int j = 0; j < W; j++) acc += (u128)G.row[(j - i + W) % W] * s[j];
        o[i] = (uint64_t)(acc % P);
    }
    memcpy(s, o, sizeof o);
}

static void permute(uint64_t *s) {
    for (int r = 0; r < ROUNDS; r++) {
        nonlinear(s);
        mds(s);
        if (r < ROUNDS - 1)
            for (int i = 0; i < W; i++) s[i] = addp(s[i], G.ark[r][i]);
    }
}

static void put_digest(const uint64_t *d, uint8_t *out) {
    for (int i = 0; i < 4; i++)
        for (int b = 0; b < 8; b++) out[8 * i + b] = (uint8_t)(d[i] >> (8 * b));
}
static uint64_t get_word(const uint8_t *b) {
    uint64_t v = 0;
    for (int i = 7; i >= 0; i--) v = (v << 8) | b[i];
    return v;
}

/* n canonical elements -> 4 canonical digest words */
static void hash_elements(const uint64_t *e, uint64_t n, uint64_t *d) {
    uint64_t s[W] = {0};
    if (n % 4) s[4] = 1;
    int i = 0;
    for (uint64_t k = 0; k < n; k++) {
        s[i] = addp(s[i], e[k] % P);
        if (++i == 4) {
            permute(s);
            i = 0;
        }
    }
    if (i) {
        s[i] = 1;
        for (int k = i + 1; k < 4; k++) s[k] = 0;
        permute(s);
    }
    memcpy(d, s, 4 * sizeof(uint64_t));
}

static void jive(const uint64_t *init_in, uint64_t *d) {
    uint64_t init[W], fin[W];
    for (int i = 0; i < W; i++) fin[i] = init[i] = init_in[i] % P;
    permute(fin);
    for (int i = 0; i < 4; i++) d[i] = addp(addp(init[i], init[4 + i]), addp(fin[i], fin[4 + i]));
}

static void merge_bytes(const uint8_t *a, const uint8_t *b, uint8_t *out) {
    uint64_t w[W], d[4];
    for (int i = 0; i < 4; i++) {
        w[i] = get_word(a + 8 * i);
        w[4 + i] = get_word(b + 8 * i);
    }
    jive(w, d);
    put_digest(d, out);
}

void gfr_permute(uint64_t *state) {
    for (int i = 0; i < W; i++) state[i] %= P;
    permute(state);
}

void gfr_merge(const uint8_t *a, const uint8_t *b, uint8_t *out) { merge_bytes(a, b, out); }

void gfr_merge_with_int(const uint8_t *seed, uint64_t v, uint8_t *out) {
    uint64_t w[W] = {0}, d[4];
    for (int i = 0; i < 4; i++) w[i] = get_word(seed + 8 * i);
    w[4] = v % P;
    if (v < P) {
        w[7] = 5;
    } else {
        w[5] = v / P;
        w[7] = 6;
    }
    jive(w, d);
    put_digest(d, out);
}

/* ---- work split over threads: job(lo, hi) on [0, n) */
typedef struct {
    void (*job)(uint64_t, uint64_t, void *);
    uint64_t lo, hi;
    void *arg;
} slice_t;
static void *run_slice(void *p) {
    slice_t *s = (slice_t *)p;
    s->job(s->lo, s->hi, s->arg);
    return 0;
}
static void split(uint64_t n, void (*job)(uint64_t, uint64_t, void *), void *arg) {
    int t = n < 256 ? 1 : MAX_THREADS;
    pthread_t th[MAX_THREADS];
    slice_t sl[MAX_THREADS];
    int started[MAX_THREADS] = {0};
    for (int k = 0; k < t; k++) {
        sl[k].job = job;
        sl[k].lo = n * (uint64_t)k / (uint64_t)t;
        sl[k].hi = n * (uint64_t)(k + 1) / (uint64_t)t;
        sl[k].arg = arg;
        if (k == t - 1 || pthread_create(&th[k], 0, run_slice, &sl[k]) != 0) run_slice(&sl[k]);
        else started[k] = 1;
    }
    for (int k = 0; k < t; k++)
        if (started[k]) pthread_join(th[k], 0);
}

typedef struct {
    const uint64_t *rows;
    uint64_t len;
    uint8_t *out;
} rows_t;
static void rows_job(uint64_t lo, uint64_t hi, void *p) {
    rows_t *a = (rows_t *)p;
    uint64_t *e = (uint64_t *)malloc((a->len ? a->len : 1) * sizeof(uint64_t)), d[4];
    for (uint64_t j = lo; j < hi; j++) {
        for (uint64_t k = 0; k < a->len; k++) e[k] = mulp(a->rows[j * a->len + k] % P, G.r_inv);
        hash_elements(e, a->len, d);
        put_digest(d, a->out + 32 * j);
    }
    free(e);
}
void gfr_hash_rows(const uint64_t *rows, uint64_t n, uint64_t len, uint8_t *out) {
    rows_t a = {rows, len, out};
    split(n, rows_job, &a);
}

typedef struct {
    const uint8_t *children;
    uint8_t *parents;
} level_t;
static void level_job(uint64_t lo, uint64_t hi, void *p) {
    level_t *a = (level_t *)p;
    for (uint64_t i = lo; i < hi; i++) merge_bytes(a->children + 64 * i, a->children + 64 * i + 32, a->parents + 32 * i);
}
/* MerkleTree::nodes: nodes[0] = zero, nodes[1] = root, nodes[i] = merge(nodes[2i], nodes[2i+1]); n a power of two >= 2 */
void gfr_merkle_nodes(const uint8_t *leaves, uint64_t n, uint8_t *nodes) {
    const uint8_t *children = leaves;
    for (uint64_t width = n / 2; width >= 1; width /= 2) {
        level_t a = {children, nodes + 32 * width};
        split(width, level_job, &a);
        children = nodes + 32 * width;
    }
    memset(nodes, 0, 32);
}

/* the smallest nonce of [begin, begin + span) whose digest's first word has `factor` trailing zero bits; span never wraps */
typedef struct {
    const uint8_t *seed;
    uint64_t mask, begin;
    uint64_t first[MAX_THREADS + 1]; /* per slice: offset of its first hit, or ~0 */
    uint64_t lo[MAX_THREADS + 1];
} grind_t;
static void grind_job(uint64_t lo, uint64_t hi, void *p) {
    grind_t *a = (grind_t *)p;
    int slot = 0;
    while (a->lo[slot] != lo) slot++;
    for (uint64_t k = lo; k < hi; k++) {
        uint8_t d[32];
        gfr_merge_with_int(a->seed, a->begin + k, d);
        if ((get_word(d) & a->mask) == 0) {
            a->first[slot] = k;
            return;
        }
    }
}
int gfr_grind(const uint8_t *seed, uint32_t factor, uint64_t begin, uint64_t span, uint64_t *nonce, uint8_t *out) {
    const uint64_t block = 8192;
    grind_t a;
    a.seed = seed;
    a.mask = factor >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << factor) - 1);
    for (uint64_t done = 0; done < span; done += block) {
        const uint64_t n = span - done < block ? span - done : block;
        const int t = n < 256 ? 1 : MAX_THREADS;
        a.begin = begin + done;
        for (int k = 0; k <= MAX_THREADS; k++) {
            a.first[k] = ~(uint64_t)0;
            a.lo[k] = k < t ? n * (uint64_t)k / (uint64_t)t : ~(uint64_t)0; /* the slices split() makes */
        }
        split(n, grind_job, &a);
        for (int k = 0; k < t; k++) {
            if (a.first[k] != ~(uint64_t)0) {
                *nonce = a.begin + a.first[k];
                gfr_merge_with_int(seed, *nonce, out);
                return 1;
            }
        }
    }
    return 0;
}
