// Part of stitch_kernels.hpp (included there, inside namespace sk): the pair description of a batched launch and the range-checked
// raw-buffer accesses (a byte offset beyond a plane reads as 0) that the projection, the source-fused sweeps and the collapse share.
// ---- S1: compose = warp + move + value cast, straight into the level-0 planes -------------------------------
// ImageProcess.cpp:218-224 + :680-681.  Level-0 planes of pair b: [a0 a1 a2 b0 b1 b2 mask], pitched, plane
// stride ps, pairs stacked (7*ps apart).  The zero canvases of the reference are implicit: an out-of-range pixel
// is written as 0.  A launch covers every pair of the batch (blockIdx.z = pair).
template <typename PX>
struct PairArgs {
    const PX* frame[MAXB];
    const PX* mosaic[MAXB];
    PX* out[MAXB];
    MapP map[MAXB];
    int fw[MAXB], fh[MAXB], mw[MAXB], mh[MAXB], ox[MAXB], oy[MAXB];
    float offx[MAXB], offy[MAXB];
    // 0: `frame` is warped through the map (sampled through k_src_index's index plane when level 0 is source-fused).
    // 1 (stitch_blend_*: both canvases are given dense, already warped / moved): `frame` IS canvas a -- plane q < 3 at (x, y)
    // is frame[q][y][x] as it stands (fw x fh = the canvas), exactly like the mosaic with a zero shift; there is no map and
    // no index plane.  One value for the whole launch.
    int a_dense;
    // The slot whose index plane (and `zi` bytes) pair i reads: i itself, or an earlier pair of the call with the same map, offsets,
    // frame size and pixel size (k_index_keys, k_compose.inc).  Written by set_index_owners alone, for every PairArgs that is built.
    int idx_pr[MAXB];
};
// idx_pr of the n pairs of a call: owner[i], or every pair its own owner (owner == nullptr: the band path, stitch_blend_*)
template <typename PX>
inline void set_index_owners(PairArgs<PX>& pa, int n, const int* owner) {
    for (int i = 0; i < MAXB; ++i) pa.idx_pr[i] = owner && i < n ? owner[i] : i;
}

// Range-checked gathers of input samples: a raw buffer descriptor over one channel plane; a byte offset beyond the
// plane (the index plane's "outside") reads as 0, which is the reference's untouched zero canvas.
template <typename PX>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t plane_rsrc(const PX* plane, size_t elems) {
    // the inputs ARE wave-uniform (kernel arguments indexed by block-derived scalars); readfirstlane makes that provable,
    // otherwise every buffer load is wrapped in a waterfall loop
    const unsigned long long a = reinterpret_cast<unsigned long long>(plane);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    const unsigned bytes = __builtin_amdgcn_readfirstlane((unsigned)(elems * sizeof(PX)));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<PX*>(((unsigned long long)hi << 32) | lo), (short)0, (int)bytes, 0x00020000);
}
template <typename PX>
__device__ __forceinline__ float buf_px(__amdgpu_buffer_rsrc_t r, unsigned byte_off);
template <>
__device__ __forceinline__ float buf_px<float>(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0));
}
template <>
__device__ __forceinline__ float buf_px<uint8_t>(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    return (float)__builtin_amdgcn_raw_buffer_load_b8(r, byte_off, 0, 0);
}
// the same loads, value left as raw bits (converted where it is consumed, so that nothing waits on the load early)
template <typename PX>
__device__ __forceinline__ float buf_raw(__amdgpu_buffer_rsrc_t r, unsigned byte_off);
template <>
__device__ __forceinline__ float buf_raw<float>(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0));
}
template <>
__device__ __forceinline__ float buf_raw<uint8_t>(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    return __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b8(r, byte_off, 0, 0));
}
template <typename PX>
__device__ __forceinline__ float raw_to_px(float raw);
template <>
__device__ __forceinline__ float raw_to_px<float>(float raw) {
    return raw;
}
template <>
__device__ __forceinline__ float raw_to_px<uint8_t>(float raw) {
    return (float)__float_as_uint(raw);
}
// "outside": a byte offset no plane reaches (the host keeps planes below 0xfffffff0 bytes), aligned for the access
template <typename PX>
__device__ __forceinline__ constexpr unsigned off_outside() {
    return 0u - (unsigned)sizeof(PX);
}
