// The rule that turns a level-0 index plane into 16-byte runs and patches (k_src_runs, k_compose.inc; include/stitch_src_runs.h),
// in one place for the kernel that applies it and for the host function that restates it.  Plain C++: a host-only program may
// include this file without the HIP headers.
#ifndef STITCH_SRC_RUNS_RULE_H
#define STITCH_SRC_RUNS_RULE_H
#include <stdint.h>
#if defined(__HIPCC__)
#define SR_HD __host__ __device__
#else
#define SR_HD
#endif

namespace src_runs {
constexpr int SR_TS = 64;                   // tile side (TS)
constexpr unsigned SR_MAX_PATCHES = 64;     // records of a tile's patch block: one per lane
constexpr unsigned SR_GENERAL = 255;        // class byte: the tile is gathered through the full index plane
constexpr unsigned SR_BASE_OUTSIDE = 0u - 16u;  // "outside" for a 16-byte access: all four words lie beyond any plane (planes stay below 0xfffffff0 bytes)

// A group is four horizontally adjacent samples, the first at a column that is a multiple of 4, with plane byte offsets o[0..3]
// (`out` = off_outside<PX>() where the sample lies outside the frame).  Its base is the offset of its first sample, usable only
// where all 16 bytes behind it lie inside the channel plane of plane_bytes bytes.
SR_HD inline unsigned group_base(unsigned o0, unsigned out, unsigned plane_bytes) {
    return o0 != out && plane_bytes >= 16u && o0 <= plane_bytes - 16u ? o0 : SR_BASE_OUTSIDE;
}
// sample j of the group is not what the 16-byte load at `base` delivers for it (zero under an outside base): one patch record
SR_HD inline bool is_patch(unsigned base, int j, unsigned oj, unsigned out, unsigned px) {
    return base == SR_BASE_OUTSIDE ? oj != out : oj != base + (unsigned)j * px;
}
SR_HD inline unsigned tile_class(unsigned patches, unsigned px) { return px != 4u || patches > SR_MAX_PATCHES ? SR_GENERAL : patches; }

// ---- the host's restatement (stitch_src_run_classes) ---------------------------------------------------------------------------
// map_to_src of k_geometry.inc: double arithmetic in the reference's order, no contraction (the library is built -ffp-contract=off;
// so must be any program that includes this)
inline bool host_map_to_src(const double p[8], float fx, float fy, int sw, int sh, int& nx, int& ny) {
    const double dx = (double)fx, dy = (double)fy;
    const float X = (float)(p[0] * dx + p[1] * dy + p[2] * dx * dy + p[3]);
    const float Y = (float)(p[4] * dx + p[5] * dy + p[6] * dx * dy + p[7]);
    if (!(X > -2147483648.0f && X < 2147483648.0f) || !(Y > -2147483648.0f && Y < 2147483648.0f)) return false;
    nx = (int)X;
    ny = (int)Y;
    return nx >= 0 && nx < sw && ny >= 0 && ny < sh;
}
// Classes of the 64x64 tiles of a cw x ch canvas, row bands outermost: cls[band * NC + t] (may be null) = 0..64 patches, 255 general;
// counts = tiles wholly outside the frame / 0 patches / 1..64 / general (an outside tile counts as outside alone).
// px = bytes per sample (4: float frames; 1: byte frames, every tile that touches the frame is general).
inline void host_classes(const double p[8], float offx, float offy, int fw, int fh, int cw, int ch, unsigned px, uint32_t counts[4], uint8_t* cls) {
    const int NC = (cw + SR_TS - 1) / SR_TS, NR = (ch + SR_TS - 1) / SR_TS;
    const unsigned out = 0u - px, plane_bytes = (unsigned)fw * (unsigned)fh * px;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    for (int b = 0; b < NR; ++b)
        for (int t = 0; t < NC; ++t) {
            unsigned patches = 0;
            bool any = false;
            for (int r = 0; r < SR_TS; ++r)
                for (int g = 0; g < SR_TS / 4; ++g) {
                    unsigned o[4];
                    for (int j = 0; j < 4; ++j) {
                        const int x = t * SR_TS + 4 * g + j, y = b * SR_TS + r;
                        int nx, ny;
                        o[j] = out;
                        if (x < cw && y < ch && host_map_to_src(p, (float)x + offx, (float)y + offy, fw, fh, nx, ny))
                            o[j] = ((unsigned)ny * (unsigned)fw + (unsigned)nx) * px;
                        any = any || o[j] != out;
                    }
                    const unsigned base = group_base(o[0], out, plane_bytes);
                    for (int j = 0; j < 4; ++j) patches += is_patch(base, j, o[j], out, px) ? 1u : 0u;
                }
            const unsigned c = tile_class(patches, px);
            if (cls) cls[(size_t)b * NC + t] = (uint8_t)c;
            ++counts[!any ? 0 : c == 0 ? 1 : c == SR_GENERAL ? 3 : 2];
        }
}
}  // namespace src_runs
#endif
