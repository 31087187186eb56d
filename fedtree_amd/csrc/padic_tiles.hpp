// LDS tile image of fthe_padic_m37 (gen_padic_mfma.py): the A operands of its two matrix-core Barrett
// products, for one prime P (or P = n for the Paillier-1024 public form) of 1009..1030 bits.
// Restates tools/padic_mfma_model.py MfmaKey.tile_image exactly (tests/test_padic_mfma_model.py compares
// the two byte for byte).
//
//   product 1 (quotient, columns s = 128..271 of q1 mu, matrix rows to 287): A1[s][i] = mu'[s - i] for
//     i < 136 (the lane's q1 bytes, fed as b - 128), A1[s][136] = g1'[s - 128] (the constant digit 1 of the B
//     operand), 0 above;
//     g1 = (128 mu sum_{i<136} 256^i - 2^1046) >> 1024: the -128 offset's correction and the truncation bias
//     (8 kS1Lo + 22 bits: the columns below kS1Lo and the shift drop less than 2^(8 kS1Lo + 14), so the
//     numerator the kernel forms lies in (q1 mu - 2^1047, q1 mu); build(P, 112) gives the window of the
//     kernel's s1lo112 variant, columns 112..271 with a bias of 2^918);
//     A1[s][137] = mu'[s - 3]: the B digit 16 c there adds c 2^28 mu for the bit 28 of q1's lowest limb;
//   product 2 (remainder; matrix column s = 1 + the column of q3 P, s = 0..159): A2[s][0] = g2'[s - 1]
//     (constant digit), A2[s][i] = P'[s - i] for i >= 1 (q3's bytes from digit 1: a plain Toeplitz
//     matrix); g2 = 128 P sum_{j<132} 256^j mod 2^1040;
//   x' = balanced base-256 digits of x (each in [-128, 127], same value).
// Tile t (1 KB): lane l's 16 bytes at l * 16 are row r = l & 31, digits i = 16 (l >> 5) + j (the
// v_mfma_i32_32x32x32_i8 A map).  Order: product 1 Toeplitz m - k = -3..1 (k <= 3), product 1 k = 4 for
// m = 0..4, product 2 k = 0 for m = 0..4, product 2 Toeplitz m - k = 0..3 (k >= 1).  19 tiles, padded to
// 20 KB (the kernel's LDS fill).  build(P, 128, 8) is the image of fthe_padic_m37s (see build).
// build_limb(P) is the image of fthe_padic_m37l, whose product 1 is fed q1's radix-2^28 limbs as they lie (see there).
#pragma once
#include <gmp.h>
#include <cstdint>
#include <vector>

namespace padic_tiles {

constexpr int kTiles = 19, kImageBytes = 20 * 1024, kS1Lo = 128, kNq1 = 136, kConst1 = 136, kNq3 = 132, kQShift = 8;
// fthe_padic_m37l: 15 product-1 tiles and product 2's nine; kLimbPad pad dwords in front of the 38 limbs; the
// constant digit in byte 3 of limb 37; P of at most kLimbMaxBits bits (the four-tile body's range)
constexpr int kLimbTiles = 24, kLimbImageBytes = 24 * 1024, kLimbPad = 1, kLimbConst = 4 * (kLimbPad + 37) + 3,
              kLimbMaxBits = 1027;

// n balanced base-256 digits of x >= 0; false if they do not hold x
inline bool balanced(const mpz_t x, int n, std::vector<int> &d) {
    mpz_t t;
    mpz_init_set(t, x);
    d.assign(n, 0);
    int c = 0;
    for (int k = 0; k < n; k++) {
        int v = (int)(mpz_get_ui(t) & 255u) + c;
        mpz_fdiv_q_2exp(t, t, 8);
        if (v >= 128) { d[k] = v - 256; c = 1; } else { d[k] = v; c = 0; }
    }
    bool ok = mpz_sgn(t) == 0 && c == 0;
    mpz_clear(t);
    return ok;
}

// 128 * x * sum_{i<n} 256^i = 128 * x * (256^n - 1) / 255
inline void offset_sum(mpz_t out, const mpz_t x, int n) {
    mpz_t g;
    mpz_init(g);
    mpz_ui_pow_ui(g, 256, (unsigned long)n);
    mpz_sub_ui(g, g, 1);
    mpz_divexact_ui(g, g, 255);
    mpz_mul(out, g, x);
    mpz_mul_ui(out, out, 128);
    mpz_clear(g);
}

// the image for P (K = 37 digits: P of 1009..1030 bits); empty on failure.  s1lo: product 1's first column.
// qshift = kQShift (fthe_padic_m37s, s1lo = 128): product 1's operand byte i is fed at digit index i + 8, so
// A1[s][i] = mu'[s - i + 8] for 8 <= i < 144, the constant digits sit at 144 and 145, and the columns i < 8 (the
// operand's pad) and i > 145 are zero.  The tiles with m - k = 1 are then zero (s - i + 8 >= 137 > 133, mu's last
// digit) and leave the image; tile (0, 0), which holds the pad columns and so is no instance of the m - k = 0
// Toeplitz tile, takes their slot (tile 4).  Product 2's tiles are the same.
inline std::vector<uint8_t> build(const mpz_t P, int s1lo = kS1Lo, int qshift = 0) {
    std::vector<uint8_t> img;
    if (mpz_sizeinbase(P, 2) < 1009 || mpz_sizeinbase(P, 2) > 1030) return img;
    if (s1lo != 112 && s1lo != 128) return img;
    if (qshift != 0 && (qshift != kQShift || s1lo != 128)) return img;
    mpz_t mu, c, b;
    mpz_inits(mu, c, b, nullptr);
    mpz_set_ui(mu, 1);
    mpz_mul_2exp(mu, mu, 56 * 37);
    mpz_fdiv_q(mu, mu, P);
    std::vector<int> mud, pd, g1, g2;
    bool ok = balanced(mu, 135, mud) && balanced(P, 130, pd);
    offset_sum(c, mu, kNq1);
    mpz_set_ui(b, 1);
    mpz_mul_2exp(b, b, 8 * s1lo + 22);
    mpz_sub(c, c, b);
    mpz_fdiv_q_2exp(c, c, 8 * s1lo);
    ok = ok && balanced(c, 160, g1);
    offset_sum(c, P, kNq3);
    mpz_fdiv_r_2exp(c, c, 1040);
    ok = ok && balanced(c, 131, g2);
    mpz_clears(mu, c, b, nullptr);
    if (!ok) return img;
    g2.resize(130);
    auto a1 = [&](int s, int i) -> int {
        i -= qshift;
        if (i < 0) return 0;
        if (i == kConst1) return (s >= s1lo && s < s1lo + 160) ? g1[s - s1lo] : 0;
        if (i == kConst1 + 1) {                 // 16 c, c = bit 28 of q1's lowest limb: mu' shifted 3 bytes
            int j = s - 3;
            return (j >= 0 && j < (int)mud.size()) ? mud[j] : 0;
        }
        if (i > kConst1) return 0;
        int j = s - i;
        return (j >= 0 && j < (int)mud.size()) ? mud[j] : 0;
    };
    auto a2 = [&](int s, int i) -> int {
        if (i == 0) return (s >= 1 && s <= (int)g2.size()) ? g2[s - 1] : 0;
        int j = s - i;
        return (j >= 0 && j < (int)pd.size()) ? pd[j] : 0;
    };
    img.reserve(kImageBytes);
    auto tile = [&](int prod, int s_base, int m, int k) {
        for (int l = 0; l < 64; l++) {
            const int r = l & 31, h = l >> 5;
            for (int j = 0; j < 16; j++) {
                const int s = s_base + 32 * m + r, i = 32 * k + 16 * h + j;
                img.push_back((uint8_t)((prod == 1 ? a1(s, i) : a2(s, i)) & 255));
            }
        }
    };
    if (qshift) {
        for (int d = -3; d <= 0; d++) tile(1, s1lo, d + 3, 3);
        tile(1, s1lo, 0, 0);
    } else {
        for (int d = -3; d <= 1; d++) tile(1, s1lo, d >= 0 ? d : 0, d >= 0 ? 0 : -d);
    }
    for (int m = 0; m < 5; m++) tile(1, s1lo, m, 4);
    for (int m = 0; m < 5; m++) tile(2, 0, m, 0);
    for (int d = 0; d <= 3; d++) tile(2, 0, d + 1, 1);
    img.resize(kImageBytes, 0);
    return img;
}

// the image of fthe_padic_m37l (tools/padic_mfma_model.py MfmaKey(P, limb_op=True).tile_image()): product 1's digit
// index 4 (t + kLimbPad) + j is byte j of q1's limb t, at bit e = 28 t + 8 j of q1, so A1[s][.] is the balanced digit
// s - e / 8 of mu 2^(e mod 8) -- of mu for even t, of 16 mu for odd t; bytes 0..2 are fed as b - 128 and byte 3 as it
// is, so g1 = (128 mu sum_{t<38, j<3} 2^(28 t + 8 j) - 2^1046) >> 1024, in the column of kLimbConst (byte 3 of limb
// 37, which is always zero).  The band is tilted (7 bits per digit index, 8 per column), so each of the 15 tiles
// with k >= m has a slot of its own, m-major; every other product-1 tile is zero.  Product 2's tiles follow as in
// build.  Empty on failure or for P outside 1009..kLimbMaxBits bits.
inline std::vector<uint8_t> build_limb(const mpz_t P) {
    std::vector<uint8_t> img;
    if (mpz_sizeinbase(P, 2) < 1009 || mpz_sizeinbase(P, 2) > (size_t)kLimbMaxBits) return img;
    mpz_t mu, c, b;
    mpz_inits(mu, c, b, nullptr);
    mpz_set_ui(mu, 1);
    mpz_mul_2exp(mu, mu, 56 * 37);
    mpz_fdiv_q(mu, mu, P);
    std::vector<int> mud[2], pd, g1, g2;
    bool ok = balanced(mu, 136, mud[0]) && balanced(P, 130, pd);
    mpz_mul_2exp(c, mu, 4);
    ok = ok && balanced(c, 136, mud[1]);
    mpz_set_ui(c, 0);
    for (int t = 0; t < 38; t++)
        for (int j = 0; j < 3; j++) mpz_setbit(c, 28 * t + 8 * j);
    mpz_mul(c, c, mu);
    mpz_mul_ui(c, c, 128);
    mpz_set_ui(b, 1);
    mpz_mul_2exp(b, b, 8 * kS1Lo + 22);
    mpz_sub(c, c, b);
    mpz_fdiv_q_2exp(c, c, 8 * kS1Lo);
    ok = ok && balanced(c, 160, g1);
    offset_sum(c, P, kNq3);
    mpz_fdiv_r_2exp(c, c, 1040);
    ok = ok && balanced(c, 131, g2);
    mpz_clears(mu, c, b, nullptr);
    if (!ok) return img;
    g2.resize(130);
    auto a1 = [&](int s, int i) -> int {
        const int t = i / 4 - kLimbPad, j = i % 4;
        if (t < 0 || t >= 38) return 0;
        if (i == kLimbConst) return (s >= kS1Lo && s < kS1Lo + 160) ? g1[s - kS1Lo] : 0;
        const int e = 28 * t + 8 * j, d = s - e / 8;
        const std::vector<int> &m = mud[(e % 8) / 4];
        return (d >= 0 && d < (int)m.size()) ? m[d] : 0;
    };
    auto a2 = [&](int s, int i) -> int {
        if (i == 0) return (s >= 1 && s <= (int)g2.size()) ? g2[s - 1] : 0;
        int j = s - i;
        return (j >= 0 && j < (int)pd.size()) ? pd[j] : 0;
    };
    img.reserve(kLimbImageBytes);
    auto tile = [&](int prod, int s_base, int m, int k) {
        for (int l = 0; l < 64; l++) {
            const int r = l & 31, h = l >> 5;
            for (int j = 0; j < 16; j++) {
                const int s = s_base + 32 * m + r, i = 32 * k + 16 * h + j;
                img.push_back((uint8_t)((prod == 1 ? a1(s, i) : a2(s, i)) & 255));
            }
        }
    };
    for (int m = 0; m < 5; m++)
        for (int k = m; k < 5; k++) tile(1, kS1Lo, m, k);
    for (int m = 0; m < 5; m++) tile(2, 0, m, 0);
    for (int d = 0; d <= 3; d++) tile(2, 0, d + 1, 1);
    return img;
}

}  // namespace padic_tiles
