// What host/mesh.cpp shares with the other mesh producer (host/fusion.cpp's i3d_fusion_extract_mesh): the triangulation table, the largest-component routine and
// the mesh they work on.  The PLY writer is the public i3d_write_ply.
#pragma once
#include <cstdint>
#include <vector>

namespace i3d {

constexpr int MC_STRIDE = 16;              // up to 5 triangles per configuration (15 edge ids), -1 padded like the reference's rows
struct McTables { unsigned char ntri[256]; signed char tri[256 * MC_STRIDE]; int max_tri = 0; bool ready = false; };
const McTables& tables();                  // mc_table.hpp unpacked into the byte table the kernels read

struct MeshData { std::vector<float> vertices; std::vector<uint8_t> colors; std::vector<int32_t> faces; };
// MeshUtil::removeLooseComponents + removeUnusedVertices; canon (optional): the canonical vertex of every vertex (see mesh.cpp)
void remove_loose_components(MeshData& M, const std::vector<int32_t>* canon = nullptr);

}  // namespace i3d
