// TSDF fusion on the device: the volume lives in an open-addressing hash table in HBM; one launch per frame
// for allocation and one for integration.  Launch wrappers of fusion_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace i3d {

constexpr unsigned long long FUSION_EMPTY = ~0ull;
constexpr int FUSION_COORD_OFFSET = 1 << 20;                 // voxel coordinates are packed as 21-bit offsets

struct FusionTable {                                         // slot-indexed SoA; the slot of a voxel never changes until the table grows
    unsigned long long* keys;                                // packed (x, y, z) or FUSION_EMPTY
    float* sdf; float* weight; uchar4* color;                // Voxel (sparse_voxel_grid.h:56-62), colour as R,G,B
    unsigned long long* rank;                                // (frame, pixel, ray step, block index) of the FIRST insertion in the reference's sequential order
    unsigned long long* crank;                               // centre state: ~0 never a block centre, 0 block expanded, else rank of the first visit (pending)
    unsigned long long mask;                                 // capacity - 1
};
struct FusionCam { float fx, fy, cx, cy; int w, h; };
struct FusionFrame {
    float voxel_size, truncation, depth_min, depth_max, weight_sample;
    float clip[6]; int use_clip;
    int bounds[6];                                           // computeFrustumBounds
    float c2w[16], w2c[16];
    unsigned long long frame;                                // index of this integrate() call
};

void launch_fusion_clear(hipStream_t st, FusionTable t);
void launch_fusion_rehash(hipStream_t st, FusionTable src, FusionTable dst);
void launch_erode(hipStream_t st, int w, int h, const float* in, int window, float max_diff, float* out);
void launch_normals(hipStream_t st, FusionCam cam, const float* depth, float thr, float* normals);
void launch_fusion_alloc(hipStream_t st, FusionTable t, FusionFrame f, FusionCam cam, const float* depth, unsigned long long limit, unsigned long long* count, int* overflow);
void launch_fusion_integrate(hipStream_t st, FusionTable t, FusionFrame f, FusionCam dcam, FusionCam ccam, const float* depth, const float* normals, const uint8_t* bgr);
// a frame taken out again, and taken out and put back at another pose in one pass; f.frame / out.frame = the ordinal of the frame that leaves
void launch_fusion_deintegrate(hipStream_t st, FusionTable t, FusionFrame f, FusionCam dcam, FusionCam ccam, const float* depth, const float* normals, const uint8_t* bgr);
void launch_fusion_reintegrate(hipStream_t st, FusionTable t, FusionFrame out, FusionFrame in, FusionCam dcam, FusionCam ccam, const float* depth, const float* normals,
                               const uint8_t* bgr);
// a whole volume fused into another under a rigid motion: x_dst = R x_src + t.  The sample of a lattice point k of dst is merge_sample
// (fusion_kernels.hip): the trilinear cell of src at R^T (k vs - t) on the general path, the src voxel k - m on the aligned one.
struct FusionMerge {
    double R[9], t[3];                                       // row-major rotation and translation (metres), src world -> dst world
    double tv[3];                                            // t / voxel_size: where the allocation puts the image of a src voxel
    int m[3];                                                // aligned path: the lattice translation
    int lo[3], hi[3];                                        // src's voxels with weight != 0 lie in [lo, hi) (its brick box in voxel coordinates)
    float voxel_size; float clip[6]; int use_clip;           // dst's lattice and clip box (as k_alloc_centres applies it)
    unsigned long long ordinal;                              // the ordinal the merge consumes: bits 41.. of the rank of every voxel it inserts
};
// counts[0] = slots of src with weight != 0 (the caller zeroes it before every launch); idempotent, repeated after a growth like launch_fusion_alloc
void launch_fusion_merge_alloc(hipStream_t st, FusionTable dst, FusionTable src, FusionMerge mg, bool aligned, unsigned long long limit, unsigned long long* count, int* overflow,
                               unsigned long long* counts);
// the final ranks (ordinal << 41) | position in ascending packed-key order of the voxels the merge inserted: slot_sorted is their sorted list (slot_list.hpp)
void launch_fusion_merge_rank(hipStream_t st, FusionTable t, unsigned long long ordinal, long long n, const unsigned int* slot_sorted);
// one lane per slot of dst: merge_sample, then integrate's update; counts[1] += voxels that received a sample
void launch_fusion_merge(hipStream_t st, FusionTable dst, FusionTable src, FusionMerge mg, bool aligned, unsigned long long* counts);
// n records with in-range keys into an EMPTY table that the caller has sized for them: record i is stored as given with the rank i and
// crank ~0; *count += records stored; flags[0] = 1 if a key appears twice (the later lane stores nothing), flags[1] = 1 if a probe ran round the whole table
void launch_fusion_insert_records(hipStream_t st, FusionTable t, long long n, const int* keys, const float* sdf, const float* weight, const uint8_t* rgb,
                                  unsigned long long* count, int* flags);
// stored voxels dropped by weight, distance or box: the criteria as prune_verdict (fusion_kernels.hip) reads them
struct FusionPrune {
    float min_weight, max_abs_sdf;                           // W fails when !(w > min_weight), S when fabsf(s) > max_abs_sdf
    float voxel_size; float box[6];                          // B: the clip test of the allocation on {x0,x1,y0,y1,z0,z1}
    int use_weight, use_sdf, box_mode;                       // box_mode 0 off, 1 keep the inside, 2 erase the inside
};
// criteria W and S on a stored voxel's weight and sdf (section 38.1 item 1): bit 0 = fails W, bit 1 = fails S, each only where enabled.  ONE definition for
// prune_verdict (fusion_kernels.hip) and for the nodes of i3d_fusion_components (SlotNode, slot_list.hpp; section 39.1 item 1): a node is a voxel with 0 here
__host__ __device__ inline unsigned prune_fails_ws(const FusionPrune& p, float w, float s) {
    unsigned v = 0u;
    if (p.use_weight && !(w > p.min_weight)) v |= 1u;
    if (p.use_sdf && fabsf(s) > p.max_abs_sdf) v |= 2u;
    return v;
}
// counts[5] += {stored, removed, failed W, failed S, failed B} (the caller zeroes them); the table is only read
void launch_fusion_prune_count(hipStream_t st, FusionTable t, FusionPrune p, unsigned long long* counts);
// the survivors of src moved into the CLEARED table dst, which has room for them: key, values, colour and rank as they are, crank = ~0.  remove: null, or one byte
// per slot of src, != 0 where the voxel leaves whatever p says (i3d_fusion_prune_components, section 39: p has every criterion off there)
void launch_fusion_prune_rehash(hipStream_t st, FusionTable src, FusionTable dst, FusionPrune p, const unsigned char* remove = nullptr);
// tests only: the table's state and a frame's contribution at n voxel keys
void launch_fusion_debug_voxels(hipStream_t st, FusionTable t, long long n, const int* keys, uint8_t* found, float* sdf, float* weight, uint8_t* rgb, long long* first_frame);
// tests only: sdf, weight and colour of the voxels that ARE stored at the n distinct keys overwritten; found = 0 and nothing written where the key is not stored
void launch_fusion_debug_poke_voxels(hipStream_t st, FusionTable t, long long n, const int* keys, const float* sdf, const float* weight, const uint8_t* rgb, uint8_t* found);
void launch_fusion_debug_frame_samples(hipStream_t st, FusionFrame f, FusionCam dcam, FusionCam ccam, const float* depth, const float* normals, const uint8_t* bgr, long long n,
                                       const int* keys, uint8_t* on, float* sample, float* wu, uint8_t* has_color, uint8_t* rgb);
// finish: slot_sorted is the list of the stored slots in the order of first insertion (slot_list.hpp)
void launch_fusion_keys(hipStream_t st, FusionTable t, long long m, const unsigned int* slot_sorted, int* kxyz);
void launch_fusion_positions(hipStream_t st, long long m, const unsigned int* slot_sorted, const int* order, unsigned int* visit_slot, int* pos_of_slot);
// correctSDF in a spatially sorted compact index space (see fusion_kernels.hip)
void launch_fusion_spatial_keys(hipStream_t st, FusionTable t, long long m, const unsigned int* slots, unsigned long long* skey);
void launch_fusion_compact_init(hipStream_t st, FusionTable t, long long m, const unsigned int* slot_c, const int* pos_of_slot, int* compact_of_slot, float* c_sdf, int* c_pos,
                                unsigned char* c_valid, unsigned char* c_touched);
void launch_fusion_build_nbr(hipStream_t st, FusionTable t, long long m, const unsigned int* slot_c, const int* compact_of_slot, const unsigned char* c_valid, int* nbr);
void launch_fusion_correct(hipStream_t st, FusionTable t, long long m, float voxel_size, const unsigned int* slot_c, const int* nbr, const int* c_pos, const unsigned char* c_valid,
                           const float* c_sdf, float* c_cur, unsigned char* c_upd, int* changed);
void launch_fusion_commit(hipStream_t st, long long m, const unsigned char* c_valid, const float* c_cur, const unsigned char* c_upd, float* c_sdf, unsigned char* c_touched, int* has_update);
void launch_fusion_write_back(hipStream_t st, FusionTable t, long long m, const unsigned int* slot_c, const float* c_sdf, const unsigned char* c_touched);
void launch_fusion_valid(hipStream_t st, FusionTable t, long long m, const unsigned int* visit_slot, int* flags);
void launch_fusion_export(hipStream_t st, FusionTable t, long long m, const unsigned int* visit_slot, const int* flags, const int* offsets, int* kxyz, float* sdf, float* weight, uint8_t* rgb);

}  // namespace i3d
