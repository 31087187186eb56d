// The LDS image of a matrix-core Barrett reduction (barrett_mfma.py), as fthe_addb_q152 and fthe_nadic_b76 read it:
// for the two constants c (product 1: mu, product 2: the modulus) as balanced base-256 digits c' (each in
// [-128, 127]),
//   copies: for output row m = 0..15 of an A tile, copy slot s(m) (rows 0-3, 12-15 -> 0..7, rows 4-11 -> 8..15:
//     the ds_read_b128 lane groups then hit 64 distinct banks), byte y = c'[K_m - y] with K_m = s_base + m + KO
//     (s_base: product 1's first output byte column; product 2: 0), 0 outside;
//   corrections (int32 per output column s, the MFMAs' srcC): 128 sum_{k < 4 nq} c'[s - k] over the 4 nq bytes of
//     the operand (fed as b - 128), product 1's plus the truncation bias digit at column bias_col.
// addb_image.hpp / nadicb_image.hpp add their key checks, their mu and their tails.
#pragma once
#include <gmp.h>
#include <cstdint>
#include <vector>

namespace barrett {

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

inline int copy_slot(int m) { return m < 4 ? m : m < 12 ? m + 4 : m - 8; }

inline void put32(std::vector<uint8_t> &img, int off, uint32_t u) {
    for (int b = 0; b < 4; b++) img[off + b] = (uint8_t)(u >> (8 * b));
}

struct Product { int a_off, corr_off, sbase, ko, tiles, nq; };   // copies, corrections, s_base, KO, tiles, q dwords
struct Layout { int copy; Product p[2]; int bias_col, bias_digit; };   // the bias: product 1's

// mu's and the modulus's digits (balanced()) -> the 2 x 16 shifted copies and both correction tables in img
inline void write_image(std::vector<uint8_t> &img, const Layout &L, const std::vector<int> &mud,
                        const std::vector<int> &nd) {
    for (int q = 0; q < 2; q++) {
        const Product &p = L.p[q];
        const std::vector<int> &d = q ? nd : mud;
        auto dig = [&](int i) { return (0 <= i && i < (int)d.size()) ? d[i] : 0; };
        for (int m = 0; m < 16; m++) {
            const int base = p.a_off + copy_slot(m) * L.copy, km = p.sbase + m + p.ko;
            for (int y = 0; y < L.copy; y++) img[base + y] = (uint8_t)(dig(km - y) & 255);
        }
        for (int i = 0; i < 16 * p.tiles; i++) {
            const int s = p.sbase + i;
            int32_t c = 0;
            for (int k = 0; k < 4 * p.nq; k++) c += dig(s - k);
            c *= 128;
            if (q == 0 && s == L.bias_col) c += L.bias_digit;
            put32(img, p.corr_off + 4 * i, (uint32_t)c);
        }
    }
}

}  // namespace barrett
