// The rule by which a 256-column block of the level-0 collapse reads one image or both (csrc/stitch_call_form.h: c4_step_at,
// c4_block_side, c4_side_counts), compiled by the host compiler alone and printed for tests/test_collapse_sides_host.py.
//   collapse_sides_dump xa xb [xa xb ...]
// For every range, both branches and every step position from two columns in front of the range to two blocks behind it -- whole
// columns and, for branch 0, the half column behind each -- one line:
//   branch start thr xa xb | a_only b_only both | the side of every block
#include <cstdio>
#include <cstdlib>

#include "stitch_call_form.h"

static_assert(sk::c4_block_side(0, 0, 300.0, 0, 255) == 1 && sk::c4_block_side(0, 0, 300.0, 256, 511) == 0 && sk::c4_block_side(0, 0, 300.0, 512, 767) == 2,
              "the rule is a constant expression: the kernel evaluates these lines");

int main(int argc, char** argv) {
    for (int i = 1; i + 1 < argc; i += 2) {
        const int xa = atoi(argv[i]), xb = atoi(argv[i + 1]);
        for (int branch = 0; branch < 2; ++branch)
            for (int t2 = 2 * (xa - 2); t2 <= 2 * (xb + 512); ++t2) {
                if (branch == 1 && (t2 & 1)) continue;
                const int start = t2 / 2;
                const double thr = t2 / 2.0;
                int n[3];
                sk::c4_side_counts(branch, start, thr, xa, xb, 1, n);
                std::printf("%d %d %.1f %d %d | %d %d %d |", branch, start, thr, xa, xb, n[0], n[1], n[2]);
                for (int xf = xa; xf < xb; xf += 256) std::printf(" %d", sk::c4_block_side(branch, start, thr, xf, std::min(xf + 255, xb - 1)));
                sk::c4_side_counts(branch, start, thr, xa, xb, 0, n);
                std::printf(" | %d %d %d\n", n[0], n[1], n[2]);
            }
    }
    return 0;
}
