// Per-key context of fthe_nadic_b76 (gen_nadicb.py), the parties' public-key encrypt r^n mod n^2 on base-n
// digits with matrix-core Barrett reductions by n (party.h:118-142 -> paillier.cpp:122-139).  Restates
// tools/nadicb_model.py nadicb_image exactly (tests/test_nadicb_model.py compares the bytes through
// fthe_debug_nadicb_image):
//
//   mu = floor(2^4128 / n); mu' (262) and n' (257) = balanced base-256 digits: the image of barrett_image.hpp
//   (product 1: c = mu, s_base = 260, corrections over k < 264 with -1 at s = 263, the -2^2104 truncation bias;
//   product 2: c = n, s_base 0, corrections over k < 260);
//   then n as 76 limbs of 27 bits (the kernel's CANON).
// Layout constants: gen/nadicb_layout.h, written by fedtree_amd/build.py from gen_nadicb.py.
#pragma once
#include <gmp.h>
#include <cstdint>
#include <vector>

#include "barrett_image.hpp"
#include "gen/nadicb_layout.h"

namespace nadicb {

inline bool n_ok(const mpz_t n) {
    const size_t b = mpz_sizeinbase(n, 2);
    return mpz_odd_p(n) && b >= 2041 && b <= 2048;
}

inline bool build(const mpz_t n, std::vector<uint8_t> &img) {
    if (!n_ok(n)) return false;
    mpz_t mu;
    mpz_init(mu);
    mpz_ui_pow_ui(mu, 2, kNbA + kNbC);
    mpz_fdiv_q(mu, mu, n);
    std::vector<int> mud, nd;
    const bool ok = barrett::balanced(mu, kNbNd1, mud) && barrett::balanced(n, kNbNd2, nd);
    mpz_clear(mu);
    if (!ok) return false;
    img.assign(kNbCtxBytes, 0);
    const barrett::Layout L = {kNbCopy,
                               {{kNbA1Off, kNbCorr1Off, kNbS1Base, kNbKO1, kNbTiles1, kNbNq1},
                                {kNbA2Off, kNbCorr2Off, 0, kNbKO2, kNbTiles2, kNbNq3}},
                               kNbBiasCol, kNbBiasDigit};
    barrett::write_image(img, L, mud, nd);
    mpz_t t;
    mpz_init(t);
    for (int j = 0; j < 76; j++) {                       // n limbs of 27 bits
        mpz_fdiv_q_2exp(t, n, 27 * j);
        barrett::put32(img, kNbNOff + 4 * j, (uint32_t)(mpz_get_ui(t) & ((1u << 27) - 1)));
    }
    mpz_clear(t);
    return true;
}

}  // namespace nadicb
