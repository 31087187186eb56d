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

}  // namespace mul192
