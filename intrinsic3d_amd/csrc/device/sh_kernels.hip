// K8/K9 — spatially-varying SH lighting: per-subvolume normal-equation blocks and per-voxel trilinear interpolation.
//
// Replaces the data-term assembly of LightingSVSH::estimate (lighting/lighting_svsh.cpp:196-253, SHDataCost :113-146:
// one AutoDiffCostFunction<1,9> per in-shell voxel) and LightingSVSH::computeVoxelShCoeffs / Subvolumes::interpolate
// (lighting_svsh.cpp:93-110, subvolumes.cpp:164-205, math.cpp:74-128).
//
// The data term of subvolume s is  sum_v w_v (phi_v . l_s - I_v)^2  with phi_v = albedo_v * H(n_v)  (9 SH basis terms),
// so everything Ceres needs from these rows is the 10x10 Gram block  G_s = sum_v w_v [phi_v; I_v][phi_v; I_v]^T
// (9x9 normal matrix, 9-vector right-hand side, scalar).  That rank-k update is the one GEMM-shaped piece of the whole
// path and runs on the matrix cores in fp64:  v_mfma_f64_16x16x4_f64, A = w*[phi;I] padded 10->16, B = [phi;I], 4 voxels
// per instruction, 16 instructions per 64-voxel wave tile, accumulated in registers.  One wave owns one CHUNK (SH_CHUNK_TILES tiles) of one subvolume's run of
// the sorted voxel list and stores its block; the chunks of a subvolume are added in chunk order by k_sh_gram_sum — no atomics, fixed summation order, and a single
// large subvolume (subvolume_size_sh: 0 = one global volume) is spread over as many waves as it has chunks instead of being walked by one.
// fp64 because the SH coefficients must match the reference's
// fp64 solve to 1e-4 and the 9x9 blocks are ill-conditioned when a subvolume sees a narrow range of normals.
#include "kernels.hpp"
#include "sh_kernels.hpp"

namespace i3d {

typedef double v4d __attribute__((ext_vector_type(4)));

static __device__ __host__ inline unsigned long long pack3(int x, int y, int z) {
    const long long B = 1ll << 20;
    return ((unsigned long long)(x + B) & 0x1fffffull) | (((unsigned long long)(y + B) & 0x1fffffull) << 21) | (((unsigned long long)(z + B) & 0x1fffffull) << 42);
}

static __device__ inline int lower_bound_u64(const unsigned long long* __restrict__ a, int n, unsigned long long key) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] < key) lo = mid + 1; else hi = mid; }
    return (lo < n && a[lo] == key) ? lo : -1;
}

// eligibility of a voxel for the SH data term (lighting_svsh.cpp:203-231) and its subvolume key (subvolumes.cpp:281-295)
__global__ void __launch_bounds__(256) k_sh_keys(GridView g, ShParams sp, unsigned long long* __restrict__ keys, int* __restrict__ iota) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= g.N) return;
    const int N = g.N;
    unsigned long long key = ~0ull;
    const bool valid = g.weight[s] > 0.0f;
    const double xs = g.x_sdf[s];
    if (valid && !(fabs(xs) > sp.thres_shell)) {
        const int nx = g.nbr[(size_t)NB_PX * N + s], ny = g.nbr[(size_t)NB_PY * N + s], nz = g.nbr[(size_t)NB_PZ * N + s];
        if (nx >= 0 && ny >= 0 && nz >= 0 && g.weight[nx] > 0.0f && g.weight[ny] > 0.0f && g.weight[nz] > 0.0f) {
            const float s0 = g.f_sdf[s];
            const float gx = g.f_sdf[nx] - s0, gy = g.f_sdf[ny] - s0, gz = g.f_sdf[nz] - s0;
            const float len = sqrtf(gx * gx + (gy * gy + gz * gz));
            const double alb = g.x_alb[s];
            if (len != 0.0f && !(len != len) && alb != 0.0 && alb == alb) {
                if (sp.single) key = pack3(0, 0, 0);
                else {
                    const float inv = 1.0f / sp.size;
                    const int ix = (int)floorf(((float)g.cx[s] * g.voxel_size) * inv), iy = (int)floorf(((float)g.cy[s] * g.voxel_size) * inv),
                              iz = (int)floorf(((float)g.cz[s] * g.voxel_size) * inv);
                    key = pack3(ix, iy, iz);
                }
            }
        }
    }
    keys[s] = key; iota[s] = s;
}

// every stored voxel's subvolume key (Subvolumes::generate allocates a subvolume for ANY stored voxel, subvolumes.cpp:214-224)
__global__ void __launch_bounds__(256) k_sh_all_keys(GridView g, ShParams sp, unsigned long long* __restrict__ keys) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= g.N) return;
    const float inv = 1.0f / sp.size;
    keys[s] = pack3((int)floorf(((float)g.cx[s] * g.voxel_size) * inv), (int)floorf(((float)g.cy[s] * g.voxel_size) * inv),
                    (int)floorf(((float)g.cz[s] * g.voxel_size) * inv));
}

// features of one voxel: f[0..8] = albedo * H(n), f[9] = luminance, weight w
static __device__ inline void sh_features(const GridView& g, int s, double f[10], double& w) {
    const int N = g.N;
    const float s0 = g.f_sdf[s];
    float nx = g.f_sdf[g.nbr[(size_t)NB_PX * N + s]] - s0, ny = g.f_sdf[g.nbr[(size_t)NB_PY * N + s]] - s0, nz = g.f_sdf[g.nbr[(size_t)NB_PZ * N + s]] - s0;
    const float len = sqrtf(nx * nx + (ny * ny + nz * nz));
    if (len != 0.0f) { nx /= len; ny /= len; nz /= len; }
    const double x = (double)nx, y = (double)ny, z = (double)nz, a = g.x_alb[s];
    f[0] = a; f[1] = a * y; f[2] = a * z; f[3] = a * x; f[4] = a * (x * y); f[5] = a * (y * z);
    f[6] = a * ((-(x * x)) - (y * y) + 2.0 * (z * z)); f[7] = a * (x * z); f[8] = a * ((x * x) - (y * y));
    const uchar4 c = g.color[s];
    f[9] = (double)((0.299f * (float)c.x + 0.587f * (float)c.y + 0.114f * (float)c.z) / 255.0f);   // intensity(color)/255 (lighting_svsh.cpp:233)
    const double tr = (double)g.truncation, xs = g.x_sdf[s];
    w = fmin(fmax(1.0 - fmin(fabs(xs), tr) / tr, 0.01), 1.0);                                       // sdfToWeight (operators.cpp:142-147)
}

// Gram accumulation over the subvolume-sorted list of eligible voxels [m0, m1) (a rank's slice).  Wave (sub, chunk) walks tiles [chunk * CT, (chunk + 1) * CT) of the
// subvolume's run in 64-voxel tiles and writes ITS 10 x 10 block and weight sum (part / wpart, zeroed by the caller: a wave without voxels writes nothing) — no block is
// shared by waves, nothing is added atomically, the sums of an estimate are bit-reproducible.  Round 4 gave a subvolume ONE wave (a single global volume of 2 M voxels
// = one wave walking 36 k tiles); round 3 used fp64 atomics wherever a chunk ended inside a subvolume.
constexpr int SH_CHUNK_TILES = 32;
__global__ void __launch_bounds__(256) k_sh_gram(GridView g, int m0, int m1, int S, int nchunk, int chunk0 /* first chunk of this slab */, const int* __restrict__ sorted_vox, const int* __restrict__ sorted_sub,
                                                 double* __restrict__ part /*[S][nchunk][100]*/, double* __restrict__ wpart /*[S][nchunk]*/) {
    __shared__ double feat[4][64][17];     // +1 padding: the MFMA operand read walks a column of 4 voxels x 16 features
    __shared__ double wl[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int sub = blockIdx.x * 4 + wv, chunk = blockIdx.y;          // (chunk: within the slab; chunk0 + chunk within the subvolume's run)
    if (sub >= S) return;
    // the subvolume's run of the (sorted) list, cut to the slice
    int lo = m0, hi = m1;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (sorted_sub[mid] < sub) lo = mid + 1; else hi = mid; }
    const int run0 = lo;
    hi = m1;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (sorted_sub[mid] <= sub) lo = mid + 1; else hi = mid; }
    const int run1 = lo;
    const long long c0 = (long long)run0 + (long long)(chunk0 + chunk) * (SH_CHUNK_TILES * 64);
    if (c0 >= run1) return;
    const int first = (int)c0, last = (int)((c0 + SH_CHUNK_TILES * 64 < run1) ? c0 + SH_CHUNK_TILES * 64 : run1);
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    double wtot = 0.0;
    for (int t0 = first; t0 < last; t0 += 64) {
        const int i = t0 + lane;
        double f[10], w = 0.0;
        if (i < last) { sh_features(g, sorted_vox[i], f, w); wtot += w; }
        else { for (int j = 0; j < 10; ++j) f[j] = 0.0; }
#pragma unroll
        for (int j = 0; j < 10; ++j) feat[wv][lane][j] = f[j];
#pragma unroll
        for (int j = 10; j < 16; ++j) feat[wv][lane][j] = 0.0;
        wl[wv][lane] = w;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0): LDS writes of this wave are visible to its own reads
#pragma unroll
        for (int grp = 0; grp < 16; ++grp) {
            const int vox = 4 * grp + (lane >> 4);
            const double bq = feat[wv][vox][lane & 15];
            const double aq = bq * wl[wv][vox];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aq, bq, acc, 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
    }
    const int col = lane & 15;
    double* const out = part + ((size_t)sub * nchunk + chunk) * 100;
#pragma unroll
    for (int r = 0; r < 4; ++r) { const int row = (lane >> 4) + 4 * r; if (row < 10 && col < 10) out[row * 10 + col] = acc[r]; }
    for (int o = 32; o > 0; o >>= 1) wtot += __shfl_down(wtot, o, 64);
    if (lane == 0) wpart[(size_t)sub * nchunk + chunk] = wtot;
}
// the chunks of every subvolume, added in chunk order (one thread per entry of a block; entry 100 = the weight sum)
// (`first` = 0: a later slab of chunks continues the running sums — the order of the additions is the chunk order either way)
__global__ void __launch_bounds__(128) k_sh_gram_sum(int S, int nchunk, int first, const double* __restrict__ part, const double* __restrict__ wpart, double* __restrict__ gram, double* __restrict__ wsub) {
    const int sub = blockIdx.x, e = threadIdx.x;
    if (sub >= S || e > 100) return;
    if (e < 100) { double s = first ? 0.0 : gram[(size_t)sub * 100 + e]; for (int c = 0; c < nchunk; ++c) s += part[((size_t)sub * nchunk + c) * 100 + e]; gram[(size_t)sub * 100 + e] = s; }
    else { double s = first ? 0.0 : wsub[sub]; for (int c = 0; c < nchunk; ++c) s += wpart[(size_t)sub * nchunk + c]; wsub[sub] = s; }
}

__global__ void __launch_bounds__(256) k_sh_assign(int M, const unsigned long long* __restrict__ sorted_keys, const unsigned long long* __restrict__ uniq, int S, int* __restrict__ sorted_sub) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    sorted_sub[i] = lower_bound_u64(uniq, S, sorted_keys[i]);
}

// Subvolumes::interpolate (subvolumes.cpp:164-205) + math::interpolationWeights / average (math.cpp:74-128)
__global__ void __launch_bounds__(256) k_sh_interpolate(GridView g, ShParams sp, const unsigned long long* __restrict__ uniq, int S,
                                                        const double* __restrict__ sh /*[S][9]*/, float* __restrict__ out /*[9][N]*/) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= g.N) return;
    const size_t N = g.N;
    double o[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) o[j] = 0.0;
    if (g.weight[s] > 0.0f && !(fabs(g.x_sdf[s]) > sp.thres_shell)) {
        if (sp.single) { for (int j = 0; j < 9; ++j) o[j] = sh[j]; }
        else {
            const float inv = 1.0f / sp.size;
            const float px = ((float)g.cx[s] * g.voxel_size) * inv - 0.5f, py = ((float)g.cy[s] * g.voxel_size) * inv - 0.5f, pz = ((float)g.cz[s] * g.voxel_size) * inv - 0.5f;
            const int x0 = (int)floorf(px), y0 = (int)floorf(py), z0 = (int)floorf(pz);
            const float wx = px - (float)x0, wy = py - (float)y0, wz = pz - (float)z0;
            const int dx[8] = {0, 1, 0, 0, 1, 0, 1, 1}, dy[8] = {0, 0, 1, 0, 1, 1, 0, 1}, dz[8] = {0, 0, 0, 1, 0, 1, 1, 1};
            const float w8[8] = {(1.0f - wx) * (1.0f - wy) * (1.0f - wz), wx * (1.0f - wy) * (1.0f - wz), (1.0f - wx) * wy * (1.0f - wz), (1.0f - wx) * (1.0f - wy) * wz,
                                 wx * wy * (1.0f - wz), (1.0f - wx) * wy * wz, wx * (1.0f - wy) * wz, wx * wy * wz};
            float sum_w = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int id = lower_bound_u64(uniq, S, pack3(x0 + dx[i], y0 + dy[i], z0 + dz[i]));
                const float w = id >= 0 ? w8[i] : 0.0f;
                if (w == 0.0f) continue;
                const double* v = sh + (size_t)id * 9;
                if (sum_w == 0.0f) { for (int j = 0; j < 9; ++j) o[j] = (double)w * v[j]; }
                else { for (int j = 0; j < 9; ++j) o[j] += (double)w * v[j]; }
                sum_w += w;
            }
            if (sum_w != 0.0f) { const double sc = (double)(1.0f / sum_w); for (int j = 0; j < 9; ++j) o[j] = o[j] * sc; }
        }
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) out[(size_t)j * N + s] = (float)o[j];
}

void launch_sh_keys(hipStream_t st, GridView g, ShParams sp, unsigned long long* keys, int* iota) { if (g.N > 0) k_sh_keys<<<(g.N + 255) / 256, 256, 0, st>>>(g, sp, keys, iota); }
void launch_sh_all_keys(hipStream_t st, GridView g, ShParams sp, unsigned long long* keys) { if (g.N > 0) k_sh_all_keys<<<(g.N + 255) / 256, 256, 0, st>>>(g, sp, keys); }
void launch_sh_assign(hipStream_t st, int M, const unsigned long long* sorted_keys, const unsigned long long* uniq, int S, int* sorted_sub) { if (M > 0) k_sh_assign<<<(M + 255) / 256, 256, 0, st>>>(M, sorted_keys, uniq, S, sorted_sub); }
int sh_gram_chunks(long long longest_run) { const long long per = (long long)SH_CHUNK_TILES * 64; const long long n = (longest_run + per - 1) / per; return n < 1 ? 1 : (int)n; }
// The chunk dimension runs in SLABS (round 6, advisor finding of round 5: the scratch was S x (chunks of the LONGEST subvolume) x 100 doubles — one large subvolume beside
// thousands of small ones, or one global volume of > 134 M voxels past the 65535 limit of gridDim.y, and nothing checked the launches): a slab holds at most
// sh_gram_slab_chunks(S) chunks of every subvolume (<= 128 MB of scratch, <= 32768 rows of the grid), its blocks are added to the running sums in chunk order, so the result
// does not depend on the slab size.  Returns a HIP error code.
int sh_gram_slab_chunks(int S, int nchunk, int forced_cap) {
    long long cap = (128ll << 20) / (100ll * 8ll * (long long)(S > 0 ? S : 1));
    if (cap < 1) cap = 1; if (cap > 32768) cap = 32768;
    if (forced_cap > 0) cap = forced_cap;      // tests: force several slabs on a small scene
    return (int)(cap < nchunk ? cap : nchunk);
}
// nchunk >= sh_gram_chunks(longest run of the slice); part [S * slab * 100] and wpart [S * slab] are scratch (slab = sh_gram_slab_chunks(S, nchunk, cap)), zeroed here
hipError_t launch_sh_gram(hipStream_t st, GridView g, int m0, int m1, int S, int nchunk, int slab, const int* sorted_vox, const int* sorted_sub, double* part, double* wpart, double* gram, double* wsub) {
    if (m1 <= m0 || S <= 0 || slab <= 0) return hipSuccess;
    for (int c0 = 0; c0 < nchunk; c0 += slab) {
        const int nc = nchunk - c0 < slab ? nchunk - c0 : slab;
        hipError_t e = hipMemsetAsync(part, 0, sizeof(double) * (size_t)S * nc * 100, st); if (e != hipSuccess) return e;
        e = hipMemsetAsync(wpart, 0, sizeof(double) * (size_t)S * nc, st); if (e != hipSuccess) return e;
        k_sh_gram<<<dim3((S + 3) / 4, nc), 256, 0, st>>>(g, m0, m1, S, nc, c0, sorted_vox, sorted_sub, part, wpart);
        k_sh_gram_sum<<<S, 128, 0, st>>>(S, nc, c0 == 0 ? 1 : 0, part, wpart, gram, wsub);
        e = hipGetLastError(); if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
void launch_sh_interpolate(hipStream_t st, GridView g, ShParams sp, const unsigned long long* uniq, int S, const double* sh, float* out) {
    if (g.N > 0) k_sh_interpolate<<<(g.N + 255) / 256, 256, 0, st>>>(g, sp, uniq, S, sh, out);
}

}  // namespace i3d
