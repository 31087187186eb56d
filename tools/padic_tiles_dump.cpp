// Writes the fthe_padic_m37 LDS tile image of P (hex argv[1]) to argv[2]: the host builder
// (fedtree_amd/csrc/padic_tiles.hpp) checked byte for byte against tools/padic_mfma_model.py.
// argv[3] (optional): the operand shift, 8 for the image of fthe_padic_m37s; "l" for the limb-fed image of
// fthe_padic_m37l (padic_tiles::build_limb).
#include "../fedtree_amd/csrc/padic_tiles.hpp"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv) {
    if (argc != 3 && argc != 4) return 2;
    mpz_t P;
    mpz_init_set_str(P, argv[1], 16);
    std::vector<uint8_t> img = argc == 4 && argv[3][0] == 'l'
                                   ? padic_tiles::build_limb(P)
                                   : padic_tiles::build(P, padic_tiles::kS1Lo, argc == 4 ? atoi(argv[3]) : 0);
    if (img.empty()) return 1;
    FILE *f = fopen(argv[2], "wb");
    if (!f) return 3;
    fwrite(img.data(), 1, img.size(), f);
    fclose(f);
    return 0;
}
