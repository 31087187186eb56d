// Per-key context of fthe_addb_q152 (gen_addb.py), the Paillier-2048 ciphertext add with a matrix-core
// Barrett reduction: out = x y mod N, N = n^2 (paillier.cpp:92-105).  Restates tools/addb_model.py
// addb_image exactly (tests/test_addb_model.py compares the bytes through fthe_debug_addb_image):
//
//   mu = floor(2^8200 / N); mu' (515) and N' (513) = balanced base-256 digits: the image of barrett_image.hpp
//   (product 1: c = mu, s_base = 512, KO = 64, corrections over k < 516 with -2 at s = 515, the -2^4121
//   truncation bias; product 2: c = N, s_base 0, KO = 560, corrections over k < 516);
//   then N as 128 little-endian dwords (the kernel's final conditional subtractions), then the integer 1 as a
//   128-dword row (the operand of a gathered index < 0).
// Layout constants: gen/addb_layout.h, written by fedtree_amd/build.py from gen_addb.py.
#pragma once
#include <gmp.h>
#include <cstdint>
#include <vector>

#include "barrett_image.hpp"
#include "gen/addb_layout.h"

namespace addb {

// n (n_words little-endian u32) -> the kctx bytes; false unless N = n^2 has 4095 or 4096 bits
inline bool build(const mpz_t n, std::vector<uint8_t> &img) {
    mpz_t N, mu;
    mpz_inits(N, mu, nullptr);
    mpz_mul(N, n, n);
    const size_t nb = mpz_sizeinbase(N, 2);
    bool ok = nb == 4095 || nb == 4096;
    std::vector<int> mud, Nd;
    if (ok) {
        mpz_ui_pow_ui(mu, 2, kAddbMuShift);
        mpz_fdiv_q(mu, mu, N);
        ok = barrett::balanced(mu, kAddbNd1, mud) && barrett::balanced(N, kAddbNd2, Nd);
    }
    if (ok) {
        img.assign(kAddbKctxBytes, 0);
        const barrett::Layout L = {kAddbCopy,
                                   {{kAddbA1Off, kAddbCorr1Off, kAddbS1Base, kAddbKO1, kAddbTiles1, kAddbNq1},
                                    {kAddbA2Off, kAddbCorr2Off, 0, kAddbKO2, kAddbTiles2, kAddbNq3}},
                                   kAddbBiasCol, kAddbBiasDigit};
        barrett::write_image(img, L, mud, Nd);
        size_t cnt = 0;
        mpz_export(img.data() + kAddbNOff, &cnt, -1, 4, 0, 0, N);
        img[kAddbOneOff] = 1;                                          // the row 1 (gathered index < 0)
    }
    mpz_clears(N, mu, nullptr);
    return ok;
}

}  // namespace addb
