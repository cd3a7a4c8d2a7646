/* ffh_perm.h -- the order of the shuffled training set (--data-randomize total): ONE stateless function.
 *
 * ffh_perm_index(seed, epoch, i, n) is a bijection of [0, n) for every n >= 1, a different one for every (seed, epoch).  There is
 * no permutation array and no state: position i of an epoch is mapped when it is needed, by the gather kernel
 * (csrc/batch_gather.hip), by the host loader and by the Python binding (ffmodel.shuffle_index) from this one statement, so the
 * three agree bit for bit.  Built on the counter hash of ffh_rng.h, like every random number of the project.
 *
 * CONSTRUCTION (a balanced Feistel network over 2w bits, cycle-walked into [0, n))
 *   n <= 1      returns 0.
 *   w           the smallest integer with 2^(2w) >= n;  mask = 2^w - 1.
 *   keys        key_r = ffh_hash(seed ^ FFH_PERM_SEED_XOR, 4 * epoch + r),  r = 0..3.
 *   x = i; repeat
 *       (L, R) = (x >> w, x & mask)
 *       four rounds r = 0..3 of   (L, R) <- (R, L ^ (ffh_hash(key_r, R) & mask))
 *       x = (L << w) | R
 *   until x < n.
 * A Feistel network is a bijection of [0, 2^(2w)) whatever its round function is.  Walking along the cycle of that bijection from
 * i < n until the next value below n is a bijection of [0, n), and the walk ends: the cycle through i returns to i, which is
 * below n.  There is no iteration cap.  2^(2w) < 4n, so a step lands below n with probability above 1/4; the longest walks
 * belong to n = 4^k + 1.
 *
 * WHICH SAMPLE GOES WHERE (B: global batch, `world` ranks, Bl = B / world samples per rank and batch, nb training batches)
 *   A rank stores, for the dense features and the labels, only its own slice of every batch: row j of its nb * Bl rows is
 *   slot j % Bl of batch j / Bl.  The owner of a table stores that table's ids for every sample.  So the shuffle permutes each
 *   rank's stripe of n_local = nb * Bl rows, with the SAME permutation on every rank:
 *       step k of epoch e, slot i of rank r:   p = ffh_perm_index(seed, e, k * Bl + i, n_local)
 *       dense features and label               this rank's stored row p
 *       ids of row r * Bl + i of the batch     global sample g = ffh_perm_global_sample(p, Bl, world, r)
 *                                                              = (p / Bl) * B + r * Bl + p % Bl
 *   No sample ever changes rank, so no rank needs another rank's dense features.  With one rank Bl = B and g = p: a uniform
 *   shuffle of the whole training set.  With more ranks it is a shuffle PER STRIPE, not of the whole set: a sample only meets
 *   samples that the file order put into the same slots of other ranks' stripes at the same permuted position.
 *   The held-out tail (--eval-batches) lies beyond n_local: never shuffled, never trained on.
 */
#ifndef FFH_PERM_H_
#define FFH_PERM_H_

#include "ffh_rng.h"

#define FFH_PERM_SEED_XOR 0x53485546464C4531ULL   /* "SHUFFLE1": keeps the round keys off every other stream drawn from --seed */

FFH_HD uint64_t ffh_perm_index(uint64_t seed, uint64_t epoch, uint64_t i, uint64_t n) {
  if (n <= 1) return 0;
  unsigned w = 1;
  while (w < 32 && (1ULL << (2 * w)) < n) w++;
  const uint64_t mask = (1ULL << w) - 1;
  uint64_t key[4];
  for (int r = 0; r < 4; r++) key[r] = ffh_hash(seed ^ FFH_PERM_SEED_XOR, 4 * epoch + (uint64_t)r);
  uint64_t x = i;
  do {
    uint64_t L = x >> w, R = x & mask;
    for (int r = 0; r < 4; r++) {
      const uint64_t t = L ^ (ffh_hash(key[r], R) & mask);
      L = R;
      R = t;
    }
    x = (L << w) | R;
  } while (x >= n);
  return x;
}

/* The global sample whose ids go with row p of rank `rank`'s stripe (see "which sample goes where"). */
FFH_HD int64_t ffh_perm_global_sample(int64_t p, int64_t Bl, int64_t world, int64_t rank) {
  return (p / Bl) * (Bl * world) + rank * Bl + p % Bl;
}

#endif /* FFH_PERM_H_ */
