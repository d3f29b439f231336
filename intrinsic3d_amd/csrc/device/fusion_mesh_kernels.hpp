// An indexed, welded mesh of the fusion table as it stands (i3d_fusion_extract_mesh).  Launch wrappers of fusion_mesh_kernels.hip.
#pragma once
#include "fusion_kernels.hpp"

namespace i3d {

constexpr int FUSION_MESH_CODES = 6;               // vertex codes per owner voxel: 0 the corner, 1..3 its +x/+y/+z edge, 4..5 the descending twin of +x/+y (29.1 item 4)
constexpr int FUSION_MESH_TRI_STRIDE = 16;         // the row length of the triangle table (host/mesh.cpp's MC_STRIDE)

// the stored voxels with weight != 0 in ascending packed key, and where each slot went (-1: not in the list): slot_list.hpp's SlotWeighted list and its inverse map
struct FusionMeshList { const unsigned long long* keys; const unsigned int* slot; const int* pos_of_slot; long long n; };
struct FusionMeshCounters { unsigned long long valid_cells, surface_cells, raw_triangles, degenerate_removed, rounded_corner_occurrences, corner_vertices; };

// one lane per list entry, the cell anchored there.  Count: used[6 position + code] = 1 for every vertex a triangle names, kept[i] = faces that survive, the counters.
// Emit: the same walk over the cells with kept > 0, the faces written through the scanned vertex ids at the scanned face offsets.
void launch_fusion_mesh_count(hipStream_t st, FusionTable t, FusionMeshList list, float min_weight, float voxel_size, const unsigned char* ntri, const signed char* tri,
                              unsigned char* used, int* kept, FusionMeshCounters* counters);
void launch_fusion_mesh_faces(hipStream_t st, FusionTable t, FusionMeshList list, float min_weight, float voxel_size, const unsigned char* ntri, const signed char* tri,
                              const int* kept /* of the count pass */, const long long* vertex_id /* [6 n] scanned */, const long long* face_at /* [n] scanned */, long long num_faces, int* faces);
// one lane per (position, code): a used one writes its vertex - the only writer of that vertex - at its scanned id
void launch_fusion_mesh_vertices(hipStream_t st, FusionTable t, FusionMeshList list, float voxel_size, const unsigned char* used, const long long* vertex_id,
                                 long long num_vertices, float* positions, unsigned char* colors, FusionMeshCounters* counters);

}  // namespace i3d
