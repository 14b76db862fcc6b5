// TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
//
// C-ABI wrappers around the REFERENCE's own colour transfer, compiled from transfer.cpp where it lies under the
// reference tree (nothing is copied into this repo).  The result, oracle/_ref/libref_transfer.so, exists only to pin
// oracle_transfer_u8 (tests/test_oracle_vs_reference.py) and to generate tests/golden/transfer.npz
// (tests/golden/make_transfer_goldens.py).  Built by oracle/Makefile (target `ref`).
//
// transfer.cpp uses the Win32 thread API for images taller than 16 rows; win32_shim.h supplies those names (see there).
// Reference entry points wrapped:
//   transfer::transfer(src, tem, output)          transfer.cpp:4-13   (the class's whole public behaviour)
//   transfer::RGBtoLab / LabToRGB (static, float) transfer.cpp:175-226
#include <cstdint>
#include <cstring>

#include "win32_shim.h"

#include "transfer.cpp"

#define REF_API extern "C" __attribute__((visibility("default")))

// the class holds its four float[3] statistics and nothing else (transfer.h:25-28), in the order
// meanSrc, meanTemplate, variableSrc, variableTemplate; they are private, so they are read from the object's bytes
static_assert(sizeof(transfer) == 48, "transfer is expected to hold exactly four float[3] members");

// planar 3 x sh x sw uchar in, planar out; stats12 (optional) = mean_src[3], sd_src[3], mean_tem[3], sd_tem[3]
REF_API int ref_transfer_u8(const uint8_t *src, int sw, int sh, const uint8_t *tem, int tw, int th, uint8_t *out, float *stats12) {
    CImg<unsigned char> s(src, sw, sh, 1, 3), t(tem, tw, th, 1, 3), o;
    transfer tr(s, t, o);
    if (o.width() != sw || o.height() != sh || o.depth() != 1 || o.spectrum() != 3) return -1;
    std::memcpy(out, o.data(), (size_t)sw * sh * 3);
    if (stats12) {
        float m[12];
        std::memcpy(m, &tr, sizeof m);
        for (int c = 0; c < 3; ++c) {
            stats12[c] = m[c];          // meanSrc
            stats12[3 + c] = m[6 + c];  // variableSrc (the standard deviation)
            stats12[6 + c] = m[3 + c];  // meanTemplate
            stats12[9 + c] = m[9 + c];  // variableTemplate
        }
    }
    return 0;
}

// n pixels, each through the static per-pixel function; in and out are n x 3 floats (R G B / L a b per pixel)
REF_API void ref_transfer_rgb_to_lab(const float *rgb, float *lab, long long n) {
    for (long long i = 0; i < n; ++i) transfer::RGBtoLab(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], &lab[3 * i], &lab[3 * i + 1], &lab[3 * i + 2]);
}

REF_API void ref_transfer_lab_to_rgb(const float *lab, float *rgb, long long n) {
    for (long long i = 0; i < n; ++i) transfer::LabToRGB(lab[3 * i], lab[3 * i + 1], lab[3 * i + 2], &rgb[3 * i], &rgb[3 * i + 1], &rgb[3 * i + 2]);
}
