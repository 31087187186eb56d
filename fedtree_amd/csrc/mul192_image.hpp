// Per-key context of fthe_mul192 (fthe_mul192.hip), the Paillier-3072 ciphertext product out = x y mod N,
// N = n^2 of 6081..6144 bits, with a Barrett reduction on the VALU.  Restates tools/mul192_model.py image()
// exactly (tests/test_mul192_model.py compares the bytes through fthe_debug_mul192_image):
//
//   mu = floor(2^(27 (225 + 231)) / N) as 232 limbs of 27 bits (one u32 each), then N as 232 such limbs, then N as
//   192 little-endian dwords (the kernel's final conditional subtraction).
//
// The matrix-core Barrett image of barrett_image.hpp is not used: the reduction of this kernel multiplies by mu and
// N on the VALU with the product routine of x y itself.
#pragma once
#include <gmp.h>
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <vector>

namespace mul192 {

constexpr int kWords = 192;                    // dwords of a row (2 n_words)
constexpr int kLimbBits = 27;
constexpr int kLanes = 8, kPerLane = 29;       // lanes per ciphertext, limbs per lane
constexpr int kLimbs = kLanes * kPerLane;      // 232 limbs: 6264 bits
constexpr int kShiftA = 225, kShiftB = 231;    // limbs: q = ((z >> 27 A) mu) >> 27 B
constexpr int kMuOff = 0, kNlOff = 4 * kLimbs, kNdOff = 8 * kLimbs, kCtxBytes = kNdOff + 4 * kWords;   // 2624
constexpr int kRowsPerWave = 64 / kLanes;      // 8
constexpr int kWaves = 8;                      // waves per workgroup, one workgroup per CU
constexpr int kPerWg = kWaves * kRowsPerWave;  // 64 rows

// n -> the context bytes; false unless n is odd with 96 words (3041..3072 bits)
inline bool build(const mpz_t n, std::vector<uint8_t> &img) {
    const size_t nb = mpz_sizeinbase(n, 2);
    if (!mpz_odd_p(n) || nb < 3041 || nb > 3072) return false;
    mpz_t N, mu, t;
    mpz_inits(N, mu, t, nullptr);
    mpz_mul(N, n, n);
    mpz_ui_pow_ui(mu, 2, (unsigned long)kLimbBits * (kShiftA + kShiftB));
    mpz_fdiv_q(mu, mu, N);
    img.assign(kCtxBytes, 0);
    auto limbs = [&](const mpz_t v, int off) {
        for (int j = 0; j < kLimbs; j++) {
            mpz_fdiv_q_2exp(t, v, (mp_bitcnt_t)kLimbBits * j);
            const uint32_t l = (uint32_t)(mpz_get_ui(t) & ((1u << kLimbBits) - 1));
            memcpy(img.data() + off + 4 * j, &l, 4);
        }
    };
    limbs(mu, kMuOff);
    limbs(N, kNlOff);
    size_t cnt = 0;
    mpz_export(img.data() + kNdOff, &cnt, -1, 4, 0, 0, N);
    mpz_clears(N, mu, t, nullptr);
    return true;
}

// out[g] = x[g] y[g] mod N for count (at most 2^22) rows of 192 dwords; x or y null: that operand is the integer 1.
// out may be exactly x or y.  kctx: the device copy of build()'s bytes.  Returns a hipError_t.
int launch(hipStream_t st, const uint32_t *x, const uint32_t *y, uint32_t *out, const void *kctx, size_t count, int n_cu);

// dst[g] = prod_{j < 8} src[gidx[j count + g]] mod N for count groups on fthe_gprod192 (one launch; rows and indices
// are addressed in 64 bits); gidx: 8 lists of count device indices into src, one below 0 standing for the integer 1
// (a group of none gives 1, a group of one its row reduced).  dst must not overlap src.  Returns a hipError_t.
int launch_gather(hipStream_t st, const uint32_t *src, const int64_t *gidx, uint32_t *dst, const void *kctx, size_t count,
                  int n_cu);

// ---- fthe_pow192: out[g] = x[g]^e t[g] mod N for one exponent e >= 2 shared by the batch ----
// The walk is sliding-window exponentiation over a table of odd powers, entry j = x^(2 j - 1), j = 1 ..; the host
// writes it as one byte string: byte 0 is the entry that seeds the running value, every further byte is 0 for a square
// or j for a product by entry j.  Restates tools/mul192_model.py schedule() / products() / plan() exactly.
constexpr int kPowMaxWindow = 5;
constexpr int kEntryWords = 32 * kLanes;       // a table entry: each lane's 29 limbs padded to 32 words (1,024 B)
constexpr uint64_t kPowBudget = 16384;         // products a wave runs in one launch, at most (one batch runs whole)

inline std::vector<uint8_t> pow_schedule(const mpz_t e, int w) {
    std::vector<uint8_t> s;
    for (long i = (long)mpz_sizeinbase(e, 2) - 1; i >= 0;) {
        if (!mpz_tstbit(e, (mp_bitcnt_t)i)) { s.push_back(0); i--; continue; }
        long lo = i - w + 1 > 0 ? i - w + 1 : 0;
        while (!mpz_tstbit(e, (mp_bitcnt_t)lo)) lo++;
        unsigned v = 0;
        for (long b = i; b >= lo; b--) v = 2 * v + (unsigned)mpz_tstbit(e, (mp_bitcnt_t)b);
        if (!s.empty()) s.insert(s.end(), (size_t)(i - lo + 1), 0);
        s.push_back((uint8_t)((v + 1) / 2));
        i = lo - 1;
    }
    return s;
}
// entries built: the highest one the walk uses
inline unsigned pow_entries(const std::vector<uint8_t> &s) {
    unsigned m = 1;
    for (uint8_t b : s) m = b > m ? b : m;
    return m;
}
// products per row: the base by 1, the table (x^2, then one per further entry), the walk, the tail
inline uint64_t pow_products(const std::vector<uint8_t> &s, bool tail) {
    const unsigned E = pow_entries(s);
    return 1 + (E > 1 ? E : 0) + (s.size() - 1) + (tail ? 1 : 0);
}
// the width in 1 .. wmax with the fewest products, the smaller one on a tie
inline int pow_plan(const mpz_t e, bool tail, int wmax, std::vector<uint8_t> &sched) {
    int best = 0;
    uint64_t cost = 0;
    for (int w = 1; w <= wmax; w++) {
        std::vector<uint8_t> s = pow_schedule(e, w);
        const uint64_t c = pow_products(s, tail);
        if (!best || c < cost) { best = w; cost = c; sched.swap(s); }
    }
    return best;
}
// workgroups of a launch over count rows, and the table's bytes for w: a table per slot (workgroup, wave, octet)
inline unsigned pow_blocks(size_t count, int n_cu) {
    const size_t cu = (size_t)(n_cu > 1 ? n_cu : 1), wg = (count + kPerWg - 1) / kPerWg;
    return (unsigned)(wg < cu ? wg : cu);
}
inline size_t pow_table_bytes(size_t count, int n_cu, int w) {
    return (size_t)pow_blocks(count, n_cu) * kPerWg * ((size_t)1 << (w - 1)) * kEntryWords * 4;
}

// One call: count rows in launches of at most blocks * 64 * max(1, kPowBudget / products) rows (2^22 at most).
// x: rows of xw <= 192 words, zero-extended (read in 16-byte pieces when xw % 4 == 0 and x is 16-byte aligned); t:
// rows of 192 words or null (the integer 1); out: rows of 192 words, canonical; out may be exactly t, or exactly x
// when xw == 192.  sched: the device copy of pow_schedule()'s slen bytes, padded to whole words; table: device bytes
// of pow_table_bytes(count, n_cu, w), 16-byte aligned; entries, products: pow_entries() and pow_products() of the
// schedule.  Returns a hipError_t.
int launch_pow(hipStream_t st, const uint32_t *x, int xw, const uint32_t *t, uint32_t *out, const void *kctx,
               const uint32_t *sched, uint32_t slen, unsigned entries, uint64_t products, uint32_t *table, int w,
               size_t count, int n_cu);

// ---- fthe_horner192: out[i] = prod_{j < planes} x[j stride + i]^(2^(j sq)) mod N ----
// Horner from the top plane: the seed by 1, then per plane below it sq squarings and a product by its row.  Restates
// tools/mul192_model.py horner_products().
inline uint64_t horner_products(int planes, int sq) { return 1 + (uint64_t)(planes - 1) * ((uint64_t)sq + 1); }

// One call: count output rows, planes >= 2 and sq >= 1 the same for all of them, plane j's rows at x + j stride rows
// (stride >= count), in launches cut by launch_pow's rule (kPowBudget products per wave, 2^22 rows).  Rows of 192
// words, any value; out canonical, not overlapping x.  No scratch.  Returns a hipError_t.
int launch_horner(hipStream_t st, const uint32_t *x, size_t stride, int planes, int sq, uint32_t *out, const void *kctx,
                  size_t count, int n_cu);

// ---- fthe_inv192_up / fthe_inv192_down: the batched inverse as a radix-8 tree ----
// Level 0 is the call's count rows; level l + 1 has one row per group of 8 rows of level l, the group's product; the
// first level of at most 8 rows is the top, inverted on the host.  Restates tools/mul192_model.py inverse_levels() /
// inverse_products() / inverse_ws_bytes() exactly.
constexpr size_t kInvRadix = 8;
inline std::vector<size_t> inv_levels(size_t count) {
    std::vector<size_t> ms(1, count);
    while (ms.back() > kInvRadix) ms.push_back((ms.back() + kInvRadix - 1) / kInvRadix);
    return ms;
}
// products as the kernels run them: per level below the top 7 per group up and 14 down, 8 more per group of level 0
// for a; a tree that is the top alone multiplies its rows by a on fthe_mul192
inline uint64_t inv_products(size_t count, bool with_a) {
    const std::vector<size_t> ms = inv_levels(count);
    if (ms.size() == 1) return with_a ? count : 0;
    uint64_t p = with_a ? 8 * (uint64_t)ms[1] : 0;
    for (size_t l = 1; l < ms.size(); l++) p += 21 * (uint64_t)ms[l];
    return p;
}
// workgroups of a level's launch, one per CU at most; count <= 8: no launch
inline unsigned inv_blocks(size_t count, int n_cu) {
    if (count <= kInvRadix) return 0;
    const size_t cu = (size_t)(n_cu > 1 ? n_cu : 1), groups = (count + kInvRadix - 1) / kInvRadix,
                 wg = (groups + kPerWg - 1) / kPerWg;
    return (unsigned)(wg < cu ? wg : cu);
}
// the workspace of one tree over count rows, blocks = inv_blocks(count, n_cu): the rows of the levels above level 0
// (768 B each; count <= 8: the top's own rows), 7 prefix entries of 1,024 B per group of every level below the top,
// one parking entry per slot (workgroup, wave, octet)
inline size_t inv_ws_bytes(size_t count, unsigned blocks) {
    const std::vector<size_t> ms = inv_levels(count);
    size_t rows = ms.size() == 1 ? count : 0, groups = 0;
    for (size_t l = 1; l < ms.size(); l++) { rows += ms[l]; groups += ms[l]; }
    return rows * kWords * 4 + groups * (kInvRadix - 1) * kEntryWords * 4 + (size_t)blocks * kPerWg * kEntryWords * 4;
}

// One level up: dst[g] = prod_{j < 8} x[8 g + j] mod N for the ceil(count / 8) groups of the level's count rows (a row
// past the end: 1), canonical rows; pre receives the groups' 7 prefix entries (entry 7 g + j: x[8 g] ... x[8 g + j],
// lazy limb rows).  dst and pre must not overlap x.  Returns a hipError_t.
int launch_inv_up(hipStream_t st, const uint32_t *x, uint32_t *pre, uint32_t *dst, const void *kctx, size_t count,
                  int n_cu);
// One level down: out[8 g + j] = inv[g] prod_{i != j} x[8 g + i] (times a[8 g + j] unless a is null), canonical rows,
// with pre as launch_inv_up left it for x and inv[g] the inverse of dst[g]; park: inv_blocks(count, n_cu) x 64 entries.
// out may be exactly x or a.  Returns a hipError_t.
int launch_inv_down(hipStream_t st, const uint32_t *x, const uint32_t *a, const uint32_t *inv, uint32_t *pre,
                    uint32_t *park, uint32_t *out, const void *kctx, size_t count, int n_cu);

}  // namespace mul192
