// Stand-alone (host only): the classification rule of csrc/src_runs_rule.h for the maps listed in a file, one per line:
//   p0 .. p7 offx offy fw fh cw ch px      (floating-point fields as C99 hex floats)
// Prints per line: the four counts, then the class byte of every tile (row bands outermost) in hex.
// tests/test_src_runs_host.py builds this with -fsanitize=address,undefined and holds the output to tests/src_runs_ref.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "src_runs_rule.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char a[10][64];
    int fw, fh, cw, ch, px;
    while (std::fscanf(f, "%63s %63s %63s %63s %63s %63s %63s %63s %63s %63s %d %d %d %d %d", a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], &fw, &fh,
                       &cw, &ch, &px) == 15) {
        double p[8];
        for (int i = 0; i < 8; ++i) p[i] = std::strtod(a[i], nullptr);
        const float offx = (float)std::strtod(a[8], nullptr), offy = (float)std::strtod(a[9], nullptr);
        const int NC = (cw + 63) / 64, NR = (ch + 63) / 64;
        std::vector<uint8_t> cls((size_t)NC * NR);
        uint32_t n[4];
        src_runs::host_classes(p, offx, offy, fw, fh, cw, ch, (unsigned)px, n, cls.data());
        std::printf("%u %u %u %u ", n[0], n[1], n[2], n[3]);
        for (uint8_t c : cls) std::printf("%02x", c);
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}
