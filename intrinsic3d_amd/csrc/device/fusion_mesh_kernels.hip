// Marching cubes over the fusion table as it stands, welded and cleaned on the device:
// The stored voxels with weight != 0 come as a list in ascending packed key with its slot -> position map (slot_list.hip's SlotWeighted and k_slot_positions).
//   k_fusion_mesh_cells<EMIT>                   one lane per list entry = the cell anchored at that voxel: configuration, the triangles of k_mc_emit
//                                               (mesh_kernels.hip), every triangle corner NAMED by (owner position, code) instead of written as a position
//                                               (29.1 item 4), the degenerate test of host/mesh.cpp.  Count marks the named vertices and counts the surviving faces;
//                                               emit repeats the walk for the cells that kept a face and writes the faces through the scanned vertex ids
//   k_fusion_mesh_vertices                      one lane per (position, code): the position and colour of a used vertex, computed from its owner - one writer
// Compiled with -ffp-contract=off: positions and colours are the expressions of k_mc_emit bit for bit (mc_device.hpp holds the one definition), and the numpy
// statement (tests/fusion_mesh_twin.py) evaluates the same fp32 operations.  No floating-point atomics; integer counters only.
#include "fusion_mesh_kernels.hpp"
#include "fusion_hash.hpp"
#include "mc_device.hpp"

namespace i3d {
namespace {

using namespace fusion_hash;          // pack_key, unpack_key, slot_of, find_slot (fusion_hash.hpp)

constexpr int MESH_BLOCK = 256;       // 4 waves of 64
inline unsigned mesh_blocks(unsigned long long n) { return (unsigned)((n + MESH_BLOCK - 1) / MESH_BLOCK); }

// corner c of the cell of (x, y, z) in the reference's numbering (mc_device.hpp)
__device__ inline int corner_dx(int c) { return (0x33 >> c) & 1; }
__device__ inline int corner_dy(int c) { return (0x99 >> c) & 1; }
__device__ inline int corner_dz(int c) { return c >> 2; }
__device__ inline bool same3(const float (&a)[3], const float (&b)[3]) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }      // +0 == -0; no NaN gets here

template <bool EMIT>
__global__ void __launch_bounds__(MESH_BLOCK) k_fusion_mesh_cells(FusionTable t, FusionMeshList list, float min_weight, float vs, const unsigned char* __restrict__ ntri,
                                                                  const signed char* __restrict__ tri, unsigned char* __restrict__ used, int* __restrict__ kept,
                                                                  FusionMeshCounters* __restrict__ counters, const long long* __restrict__ vertex_id,
                                                                  const long long* __restrict__ face_at, long long num_faces, int* __restrict__ faces) {
    // the 8 corners of a lane's cell, one column per lane: the triangle walk indexes them by a table entry, which registers cannot do without scratch
    __shared__ int s_pos[8][MESH_BLOCK];
    __shared__ float s_sdf[8][MESH_BLOCK];
    __shared__ unsigned int s_count[5];
    const int tid = threadIdx.x;
    if (!EMIT) { if (tid < 5) s_count[tid] = 0u; __syncthreads(); }
    const long long i = (long long)blockIdx.x * MESH_BLOCK + tid;
    int idx = 0, x = 0, y = 0, z = 0;
    bool valid = i < list.n;
    if (EMIT && valid) valid = kept[i] > 0;                                           // the count pass found no surviving face here: nothing to probe for
    if (valid) {
        unpack_key(list.keys[i], x, y, z);
        valid = x + 1 < FUSION_COORD_OFFSET && y + 1 < FUSION_COORD_OFFSET && z + 1 < FUSION_COORD_OFFSET;      // the far corners have a packed key
    }
    if (valid) {
        // the home slots of the seven other corners together: an EMPTY one means the corner is not stored and the cell leaves after one round trip
        unsigned long long ck[8], home[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) { ck[c] = pack_key(x + corner_dx(c), y + corner_dy(c), z + corner_dz(c)); home[c] = c == 2 ? ck[c] : t.keys[slot_of(ck[c], t.mask)]; }
#pragma unroll
        for (int c = 0; c < 8; ++c) valid = valid && home[c] != FUSION_EMPTY;
        if (valid) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                if (!valid) break;
                const long long sl = c == 2 ? (long long)list.slot[i] : (home[c] == ck[c] ? (long long)slot_of(ck[c], t.mask) : find_slot(t, ck[c]));
                if (sl < 0) { valid = false; break; }
                const int p = c == 2 ? (int)i : list.pos_of_slot[sl];
                if (p < 0) { valid = false; break; }                                   // stored with weight 0
                const float w = t.weight[sl], s = t.sdf[sl];
                if (!(w >= min_weight) || !isfinite(s)) { valid = false; break; }     // 29.1 item 1; a NaN weight fails the comparison
                s_pos[c][tid] = p; s_sdf[c][tid] = s;
                if (s < 0.0f) idx |= 1 << c;
            }
        }
    }
    const bool surface = valid && idx != 0 && idx != 255;
    const int nt = surface ? (int)ntri[idx] : 0;
    int nkept = 0, nrounded = 0;
    long long out = 0;
    if (EMIT && surface) out = face_at[i];
    for (int k = 0; k < nt; ++k) {
        long long v[3]; float P[3][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int e = tri[idx * FUSION_MESH_TRI_STRIDE + 3 * k + j];
            const int a = mc_ea(e), b = mc_eb(e);
            const float s1 = s_sdf[a][tid], s2 = s_sdf[b][tid];
            // voxelToWorld = float(i) * voxel_size, as k_mc_emit
            const float va[3] = {(float)(x + corner_dx(a)) * vs, (float)(y + corner_dy(a)) * vs, (float)(z + corner_dz(a)) * vs};
            const float vb[3] = {(float)(x + corner_dx(b)) * vs, (float)(y + corner_dy(b)) * vs, (float)(z + corner_dz(b)) * vs};
#pragma unroll
            for (int q = 0; q < 3; ++q) P[j][q] = mc_lerp(s1, s2, va[q], vb[q]);
            const bool at_a = same3(P[j], va), at_b = same3(P[j], vb);
            if (at_a || at_b) {                                                        // a corner vertex: owner = that corner, code 0
                v[j] = (long long)FUSION_MESH_CODES * s_pos[at_a ? a : b][tid];
                const bool early = fabsf(0.0f - s1) < 0.00001f || fabsf(0.0f - s2) < 0.00001f || fabsf(s1 - s2) < 0.00001f;      // mc_lerp's three early returns
                if (!early) ++nrounded;
            } else {
                // an edge vertex: owner = the lower corner of the edge.  Edges 0,1,4,5 run DOWN their axis (from the upper corner to the lower one): the neighbouring
                // cell walks the same edge upwards and mc_lerp is not symmetric in the last bit, so the descending walk is the same vertex only where both give the
                // same coordinate (29.1 item 4)
                const int axis = e >= 8 ? 2 : ((e & 1) ? 0 : 1);
                const bool down = e < 8 && (e & 2) == 0;
                int code = axis + 1;
                if (down) {
                    const float pa = axis == 0 ? P[j][0] : P[j][1], la = axis == 0 ? va[0] : va[1], lb = axis == 0 ? vb[0] : vb[1];
                    if (!(mc_lerp(s2, s1, lb, la) == pa)) code = axis + 4;
                }
                v[j] = (long long)FUSION_MESH_CODES * s_pos[down ? b : a][tid] + code;
            }
        }
        // removeDegenerateFaces (host/mesh.cpp): an index twice, or the area 0 / NaN / inf
        bool keep = v[0] != v[1] && v[0] != v[2] && v[1] != v[2];
        if (keep) {
            const float e0[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]}, e1[3] = {P[2][0] - P[1][0], P[2][1] - P[1][1], P[2][2] - P[1][2]};
            const float cr[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
            const double area = (double)sqrtf(cr[0] * cr[0] + (cr[1] * cr[1] + cr[2] * cr[2]));
            keep = !(area == 0.0 || isnan(area) || isinf(area));
        }
        if (EMIT) {
            if (keep) {
                const long long at = out + nkept;
                if (at >= 0 && at < num_faces) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) faces[3 * at + j] = (int)vertex_id[v[j]];
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) used[v[j]] = 1;                               // every writer stores the same byte
        }
        if (keep) ++nkept;
    }
    if (!EMIT) {
        if (i < list.n) kept[i] = nkept;
        if (valid) atomicAdd(&s_count[0], 1u);
        if (surface) { atomicAdd(&s_count[1], 1u); atomicAdd(&s_count[2], (unsigned)nt); atomicAdd(&s_count[3], (unsigned)(nt - nkept)); }
        if (nrounded) atomicAdd(&s_count[4], (unsigned)nrounded);
        __syncthreads();
        if (tid < 5 && s_count[tid]) atomicAdd(&counters->valid_cells + tid, (unsigned long long)s_count[tid]);
    }
}

__global__ void __launch_bounds__(MESH_BLOCK) k_fusion_mesh_vertices(FusionTable t, FusionMeshList list, float vs, const unsigned char* __restrict__ used,
                                                                     const long long* __restrict__ vertex_id, long long num_vertices, float* __restrict__ positions,
                                                                     unsigned char* __restrict__ colors, FusionMeshCounters* __restrict__ counters) {
    const long long g = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (g >= list.n * FUSION_MESH_CODES || !used[g]) return;
    const long long id = vertex_id[g];
    if (id < 0 || id >= num_vertices) return;
    const long long p = g / FUSION_MESH_CODES; const int code = (int)(g - p * FUSION_MESH_CODES);
    int k[3]; unpack_key(list.keys[p], k[0], k[1], k[2]);
    const unsigned int sl = list.slot[p];
    const uchar4 cl = t.color[sl];
    const float inv = 1.0f / 255.0f;
    float P[3]; unsigned char col[3];
    if (code == 0) {
        P[0] = (float)k[0] * vs; P[1] = (float)k[1] * vs; P[2] = (float)k[2] * vs;
        col[0] = (unsigned char)(((float)cl.x * inv) * 255.0f); col[1] = (unsigned char)(((float)cl.y * inv) * 255.0f); col[2] = (unsigned char)(((float)cl.z * inv) * 255.0f);
        atomicAdd(&counters->corner_vertices, 1ull);
    } else {
        const int axis = (code - 1) % 3; const bool down = code >= 4;
        const int u[3] = {k[0] + (axis == 0), k[1] + (axis == 1), k[2] + (axis == 2)};
        const long long su = find_slot(t, pack_key(u[0], u[1], u[2]));
        if (su < 0) return;                                                             // cannot be: a valid cell named this vertex
        const uchar4 cu = t.color[su];
        const float s_lo = t.sdf[sl], s_up = t.sdf[su];
        const float s1 = down ? s_up : s_lo, s2 = down ? s_lo : s_up;
        const uchar4 ca = down ? cu : cl, cb = down ? cl : cu;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float lo = (float)k[q] * vs, up = (float)u[q] * vs;
            P[q] = mc_lerp(s1, s2, down ? up : lo, down ? lo : up);
        }
        col[0] = (unsigned char)(mc_lerp(s1, s2, (float)ca.x * inv, (float)cb.x * inv) * 255.0f);
        col[1] = (unsigned char)(mc_lerp(s1, s2, (float)ca.y * inv, (float)cb.y * inv) * 255.0f);
        col[2] = (unsigned char)(mc_lerp(s1, s2, (float)ca.z * inv, (float)cb.z * inv) * 255.0f);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) { positions[3 * id + q] = P[q]; colors[3 * id + q] = col[q]; }
}

}  // namespace

void launch_fusion_mesh_count(hipStream_t st, FusionTable t, FusionMeshList list, float min_weight, float voxel_size, const unsigned char* ntri, const signed char* tri,
                              unsigned char* used, int* kept, FusionMeshCounters* counters) {
    if (list.n > 0) k_fusion_mesh_cells<false><<<mesh_blocks(list.n), MESH_BLOCK, 0, st>>>(t, list, min_weight, voxel_size, ntri, tri, used, kept, counters, nullptr, nullptr, 0, nullptr);
}
void launch_fusion_mesh_faces(hipStream_t st, FusionTable t, FusionMeshList list, float min_weight, float voxel_size, const unsigned char* ntri, const signed char* tri,
                              const int* kept, const long long* vertex_id, const long long* face_at, long long num_faces, int* faces) {
    if (list.n > 0 && num_faces > 0)
        k_fusion_mesh_cells<true><<<mesh_blocks(list.n), MESH_BLOCK, 0, st>>>(t, list, min_weight, voxel_size, ntri, tri, nullptr, const_cast<int*>(kept), nullptr, vertex_id, face_at,
                                                                              num_faces, faces);
}
void launch_fusion_mesh_vertices(hipStream_t st, FusionTable t, FusionMeshList list, float voxel_size, const unsigned char* used, const long long* vertex_id,
                                 long long num_vertices, float* positions, unsigned char* colors, FusionMeshCounters* counters) {
    if (list.n > 0 && num_vertices > 0)
        k_fusion_mesh_vertices<<<mesh_blocks((unsigned long long)list.n * FUSION_MESH_CODES), MESH_BLOCK, 0, st>>>(t, list, voxel_size, used, vertex_id, num_vertices, positions, colors, counters);
}

}  // namespace i3d
