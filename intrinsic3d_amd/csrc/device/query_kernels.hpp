// The stored field at arbitrary world points and their projection onto its zero level set (query_kernels.hip, i3d_query_points / i3d_fusion_query_points).
// The definition the kernel implements is DESIGN.md section 17.
#pragma once
#include "render_kernels.hpp"

namespace i3d {

constexpr int QUERY_BLOCK = 256;                  // one lane per point
constexpr int QUERY_MAX_STEPS = 64;
constexpr double QUERY_MAX_COORD = 1048576.0;     // |p / vs| >= 2^20: no key, no lookup, no int conversion

struct QueryParams {
    long long n;
    int project, max_steps;
    double tol;                                   // tolerance_voxels * vs
};

struct QueryOut {                                 // device arrays, any may be null
    double* sdf; float* normal /*[n][3]*/; float* albedo; double* foot /*[n][3]*/; double* distance; unsigned char* status;
};

// one row per workgroup of k_query, and the total of k_query_reduce
struct QueryRow {
    double sum_abs_sdf, sum_sq_sdf, max_abs_sdf, sum_abs_distance, sum_sq_distance, max_abs_distance;
    long long valid, projected, steps;
};

inline int query_rows(long long n) { return (int)((n + QUERY_BLOCK - 1) / QUERY_BLOCK); }

// rows: [query_rows(n)] written by k_query, total: one row written by the reduction (both fully overwritten: no initialisation needed).  The grids' brick
// bitmaps are not read.
void launch_query(hipStream_t st, const RenderGrid& g, const QueryParams& p, const double* points, const QueryOut& out, QueryRow* rows, QueryRow* total);
void launch_query(hipStream_t st, const FusionRenderGrid& g, const QueryParams& p, const double* points, const QueryOut& out, QueryRow* rows, QueryRow* total);

}  // namespace i3d
