/* ORACLE (test infrastructure): a plain Rescue Prime reference over p = 2^64 - 2^32 + 1 for Rp64_256 and RpJive64_256,
 * see rescue_ref.c.  Every function takes the hasher's parameters as a block of 64-bit words, filled at run time from
 * the params.json files of tests/golden (oracle/oracle.py: rescue_params):
 *     [0] kind (ORC_RESCUE_RP = sponge with the element count in place 0, ORC_RESCUE_JIVE = padded sponge + Jive merge)
 *     [1] state width w   [2] first rate place   [3] rounds   [4] alpha   [5] inv_alpha
 *     [6 ..) MDS row (w words), ARK1 (rounds * w), ARK2 (rounds * w); all canonical integers.
 * Digests are four canonical little-endian u64 (32 bytes).  Functions return 0, or a negative number for bad parameters. */
#pragma once
#include <stddef.h>
#include <stdint.h>

#define ORC_RESCUE_RP 0
#define ORC_RESCUE_JIVE 1

/* n states of w canonical integers (any u64 is reduced mod p), permuted in place */
int orc_rescue_permute(const uint64_t *prm, uint64_t *states, size_t n, int threads);
/* n rows of `len` stored (Montgomery) residues, `stride` words apart -> n digests */
int orc_rescue_hash_rows(const uint64_t *prm, const uint64_t *rows, size_t n, size_t len, size_t stride, uint8_t *digests,
                         int threads);
/* the 8 digest words of a || b (any u64) -> digest */
int orc_rescue_merge(const uint64_t *prm, const uint64_t words[8], uint8_t out[32]);
int orc_rescue_merge_with_int(const uint64_t *prm, const uint64_t seed[4], uint64_t value, uint8_t out[32]);
/* MerkleTree::nodes for n (a power of two >= 2) leaves: nodes[0] = zero, nodes[i] = merge(nodes[2i], nodes[2i+1]) */
int orc_rescue_merkle_nodes(const uint64_t *prm, const uint8_t *leaves, size_t n, uint8_t *nodes, int threads);
/* the smallest nonce of [begin, begin + max_nonces), the range ending at 2^64 - 1 at the latest, whose
 * merge_with_int(seed, nonce) has `factor` trailing zero bits in its first word: 1 and *nonce, digest; 0 for none */
int orc_rescue_grind(const uint64_t *prm, const uint64_t seed[4], unsigned factor, uint64_t begin, uint64_t max_nonces,
                     uint64_t *nonce, uint8_t digest[32], int threads);
