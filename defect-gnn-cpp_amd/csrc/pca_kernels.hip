// pca_kernels.hip — count, mean and centred 35 x 35 scatter of a Betti block [rows][35] f64 in HBM:
// the dataset-level moments of PCA::fit (reference pca.cpp:15-34: x.rowwise() - x.colwise().mean(),
// then the SVD of the centred matrix, whose right singular vectors are the eigenvectors of this
// scatter). Two passes over the block, 280 B per row each:
//   pass 1  column sums and the count of finite rows per tile of kPcaTileRows rows -> the mean;
//   pass 2  sum over finite rows of (x - mean)(x - mean)^T per tile, upper triangle.
// A row with any non-finite value (a failed atom's NaN row) is left out of both passes by the same
// test on the raw values. Every tile writes its partial to the workspace and a second small launch
// adds the partials in a fixed order, so the result depends on the row count and the data alone:
// no floating-point atomics, no dependence on the CU count.
// Pass 2 is 630 FMA per 280-B row. A lane owns one 4 x 4 tile of the matrix padded to 36 x 36 (45
// upper tiles, 45 of a wave's 64 lanes): per row it reads 8 operands from LDS (four 16-B reads) for
// 16 FMAs, every operand reused four times from registers; the four waves of a block take row
// slices of the staged rows and are added through LDS at the end of the tile.
#include "dgn_internal.hpp"

namespace dgn {

constexpr int kPcaBlock = 256;
constexpr int kPcaWaves = kPcaBlock / 64;
constexpr int kPcaChunk = 64;      // rows staged in LDS at a time
constexpr int kPcaPad = 36;        // padded row: 9 groups of 4 columns
constexpr int kPcaLaneTiles = 45;  // upper 4 x 4 tiles of the 9 x 9 grid
constexpr int kPcaSumGroups = 7;   // pass 1: 7 row groups x 35 columns = 245 threads
constexpr int kPcaRedX = 64, kPcaRedY = 16, kPcaRedRun = 128;  // partial-sum launch (below)
static_assert(kPcaTileRows % kPcaChunk == 0 && kPcaChunk % kPcaWaves == 0, "tile / chunk / wave split");
static_assert(kPcaSumGroups * kPcaDim <= kPcaBlock, "pass-1 thread map");
static_assert((kPcaWaves - 1) * kPcaLaneTiles * 16 <= kPcaChunk * kPcaPad, "wave partials alias the staged rows");

__device__ inline bool finite_f64(double v) {
    return (__double_as_longlong(v) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll;
}

constexpr int kPcaPer = (kPcaChunk * kPcaDim + kPcaBlock - 1) / kPcaBlock;  // values of a chunk per thread

// Rows [row0, row0 + kPcaChunk) of the block, coalesced, into registers (0 past the end). Issued one
// chunk ahead: the loads of chunk k + 1 are in flight while chunk k is summed.
__device__ inline void pca_load_rows(const double* __restrict__ betti, int64_t rows, int64_t row0,
                                     double (&v)[kPcaPer]) {
    const int64_t left = rows - row0;
    const int n = (int)(left < kPcaChunk ? left : kPcaChunk) * kPcaDim;
    const double* src = betti + row0 * kPcaDim;
#pragma unroll
    for (int j = 0; j < kPcaPer; ++j) {
        const int x = threadIdx.x + j * kPcaBlock;
        v[j] = x < n ? src[x] : 0.0;
    }
}

// The loaded rows into xs (columns 0..34), centred as node_features_kernel does when kCentre.
// bad[i] = 1: row i is past the end or holds a non-finite value (tested on the raw value in either
// pass). `bad` alternates between two arrays from one chunk to the next, so the barrier after its
// reset also fences the previous chunk's reads of xs.
template <bool kCentre>
__device__ inline void pca_stage_rows(const double (&v)[kPcaPer], int64_t rows, int64_t row0, const double* mean_s,
                                      double (*xs)[kPcaPad], int* bad) {
    const int t = threadIdx.x;
    if (t < kPcaChunk) bad[t] = row0 + t >= rows;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPcaPer; ++j) {
        const int x = t + j * kPcaBlock;
        if (x < kPcaChunk * kPcaDim) {
            const int i = x / kPcaDim, c = x - i * kPcaDim;
            if (!finite_f64(v[j])) bad[i] = 1;
            xs[i][c] = kCentre && row0 + i < rows ? v[j] - mean_s[c] : v[j];  // x.rowwise() - mean
        }
    }
    __syncthreads();
}

// pass 1: part[tile][0..34] = column sums over the tile's finite rows, part[tile][35] = their count
__global__ __launch_bounds__(kPcaBlock) void pca_sums_kernel(const double* __restrict__ betti, int64_t rows,
                                                             double* __restrict__ part) {
    __shared__ double xs[kPcaChunk][kPcaPad];
    __shared__ int bad[2][kPcaChunk];
    __shared__ double red[kPcaSumGroups][kPcaSumWidth];
    const int t = threadIdx.x;
    const int g = t / kPcaDim, c = t - g * kPcaDim;  // row group, column
    const int64_t tile0 = (int64_t)blockIdx.x * kPcaTileRows;
    double s = 0.0, cnt = 0.0;
    double v[kPcaPer];
    pca_load_rows(betti, rows, tile0, v);
    for (int k = 0; k < kPcaTileRows / kPcaChunk; ++k) {
        const int64_t row0 = tile0 + (int64_t)k * kPcaChunk;
        if (row0 >= rows) break;
        const int* b = bad[k & 1];
        pca_stage_rows<false>(v, rows, row0, nullptr, xs, bad[k & 1]);
        if (k + 1 < kPcaTileRows / kPcaChunk && row0 + kPcaChunk < rows) pca_load_rows(betti, rows, row0 + kPcaChunk, v);
        if (g < kPcaSumGroups)
            for (int r = g; r < kPcaChunk; r += kPcaSumGroups)
                if (!b[r]) {
                    s += xs[r][c];
                    cnt += 1.0;
                }
    }
    if (g < kPcaSumGroups) {
        red[g][c] = s;
        if (c == 0) red[g][kPcaDim] = cnt;
    }
    __syncthreads();
    if (t < kPcaSumWidth) {
        double a = 0.0;
        for (int q = 0; q < kPcaSumGroups; ++q) a += red[q][t];
        part[(int64_t)blockIdx.x * kPcaSumWidth + t] = a;
    }
}

// pass 2: part[tile][a * 35 - a (a - 1) / 2 + (b - a)] = sum over the tile's finite rows of
// (x_a - mean_a)(x_b - mean_b), a <= b; result[1..35] = the mean of pass 1
__global__ __launch_bounds__(kPcaBlock, 4) void pca_scatter_kernel(const double* __restrict__ betti, int64_t rows,
                                                                const double* __restrict__ result,
                                                                double* __restrict__ part) {
    __shared__ __align__(32) double xs[kPcaChunk][kPcaPad];  // centred rows; the waves' partials at the end
    __shared__ int bad[2][kPcaChunk];
    __shared__ double mean_s[kPcaPad];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t < kPcaDim) mean_s[t] = result[1 + t];
    if (t < kPcaChunk) xs[t][kPcaDim] = 0.0;  // pad column (staging writes columns 0..34 only)
    // the lane's tile (ti, tj), ti <= tj, of the 9 x 9 grid in row-major order of the upper triangle
    const bool active = lane < kPcaLaneTiles;
    int ti = 0, tj = 0;
    {
        int l = active ? lane : 0, len = kPcaPad / 4;
        while (l >= len) {
            l -= len;
            ++ti;
            --len;
        }
        tj = ti + l;
    }
    double acc[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
    const int64_t tile0 = (int64_t)blockIdx.x * kPcaTileRows;
    constexpr int kSlice = kPcaChunk / kPcaWaves;  // rows of a chunk per wave
    double v[kPcaPer];
    pca_load_rows(betti, rows, tile0, v);
    for (int k = 0; k < kPcaTileRows / kPcaChunk; ++k) {
        const int64_t row0 = tile0 + (int64_t)k * kPcaChunk;
        if (row0 >= rows) break;
        const int* b = bad[k & 1];
        pca_stage_rows<true>(v, rows, row0, mean_s, xs, bad[k & 1]);
        if (k + 1 < kPcaTileRows / kPcaChunk && row0 + kPcaChunk < rows) pca_load_rows(betti, rows, row0 + kPcaChunk, v);
        if (active) {
#pragma unroll 4
            for (int r = w * kSlice; r < (w + 1) * kSlice; ++r) {
                if (b[r]) continue;  // the same row for the whole wave
                const double2 a0 = *reinterpret_cast<const double2*>(&xs[r][4 * ti]);
                const double2 a1 = *reinterpret_cast<const double2*>(&xs[r][4 * ti + 2]);
                const double2 b0 = *reinterpret_cast<const double2*>(&xs[r][4 * tj]);
                const double2 b1 = *reinterpret_cast<const double2*>(&xs[r][4 * tj + 2]);
                const double av[4] = {a0.x, a0.y, a1.x, a1.y}, bv[4] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[p][q] = __builtin_fma(av[p], bv[q], acc[p][q]);
            }
        }
    }
    __syncthreads();  // every wave is done with xs
    double* red = &xs[0][0];  // [wave - 1][entry][lane tile]
    if (active && w > 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) red[((w - 1) * 16 + e) * kPcaLaneTiles + lane] = acc[e >> 2][e & 3];
    }
    __syncthreads();
    if (active && w == 0) {
        double* o = part + (int64_t)blockIdx.x * kPcaTri;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            double v = acc[e >> 2][e & 3];
            for (int ww = 0; ww < kPcaWaves - 1; ++ww) v += red[(ww * 16 + e) * kPcaLaneTiles + lane];  // wave order
            const int a = 4 * ti + (e >> 2), bb = 4 * tj + (e & 3);
            if (a <= bb && bb < kPcaDim) o[a * kPcaDim - a * (a - 1) / 2 + (bb - a)] = v;
        }
    }
}

// out[col] = sum over tiles of part[tile][col] in a fixed order that depends on nb alone: thread row y
// adds, in index order, the tiles of the runs of kPcaRedRun tiles y, y + 16, y + 32, ...; the 16 row
// sums are then added in row order. With want_mean (width 36, one block): out[0] = n and
// out[1 + c] = sum_c / n (0 when n == 0) instead.
__global__ __launch_bounds__(kPcaRedX* kPcaRedY) void pca_reduce_kernel(const double* __restrict__ part, int64_t nb,
                                                                         int width, double* __restrict__ out,
                                                                         int want_mean) {
    __shared__ double acc_s[kPcaRedY][kPcaRedX];
    const int x = threadIdx.x, y = threadIdx.y;
    const int col = blockIdx.x * kPcaRedX + x;
    double a = 0.0;
    if (col < width)
        for (int64_t g0 = (int64_t)y * kPcaRedRun; g0 < nb; g0 += (int64_t)kPcaRedY * kPcaRedRun) {
            const int64_t g1 = g0 + kPcaRedRun < nb ? g0 + kPcaRedRun : nb;
#pragma unroll 8
            for (int64_t b = g0; b < g1; ++b) a += part[b * width + col];
        }
    acc_s[y][x] = a;
    __syncthreads();
    if (y == 0) {
        double v = 0.0;
        for (int q = 0; q < kPcaRedY; ++q) v += acc_s[q][x];
        if (!want_mean) {
            if (col < width) out[col] = v;
        } else {
            acc_s[0][x] = v;  // only this thread reads acc_s[..][x] above
        }
    }
    if (!want_mean) return;
    __syncthreads();
    if (y == 0 && x < kPcaSumWidth) {
        const double n = acc_s[0][kPcaDim];
        if (x == kPcaDim) out[0] = n;
        else out[1 + x] = n > 0.0 ? acc_s[0][x] / n : 0.0;
    }
}

hipError_t launch_pca_sums(hipStream_t s, const double* betti, int64_t rows, double* workspace) {
    const int64_t nb = pca_tiles(rows);
    if (nb <= 0) return hipSuccess;
    if (nb > INT32_MAX) return hipErrorInvalidValue;
    double* part = workspace;
    double* result = workspace + nb * (kPcaSumWidth + kPcaTri);
    hipLaunchKernelGGL(pca_sums_kernel, dim3((unsigned)nb), dim3(kPcaBlock), 0, s, betti, rows, part);
    hipLaunchKernelGGL(pca_reduce_kernel, dim3(1), dim3(kPcaRedX, kPcaRedY), 0, s, part, nb, kPcaSumWidth, result, 1);
    return hipGetLastError();
}

hipError_t launch_pca_scatter(hipStream_t s, const double* betti, int64_t rows, double* workspace) {
    const int64_t nb = pca_tiles(rows);
    if (nb <= 0) return hipSuccess;
    if (nb > INT32_MAX) return hipErrorInvalidValue;
    double* part = workspace + nb * kPcaSumWidth;
    double* result = workspace + nb * (kPcaSumWidth + kPcaTri);
    hipLaunchKernelGGL(pca_scatter_kernel, dim3((unsigned)nb), dim3(kPcaBlock), 0, s, betti, rows, result, part);
    hipLaunchKernelGGL(pca_reduce_kernel, dim3((kPcaTri + kPcaRedX - 1) / kPcaRedX), dim3(kPcaRedX, kPcaRedY), 0, s,
                       part, nb, kPcaTri, result + 1 + kPcaDim, 0);
    return hipGetLastError();
}

}  // namespace dgn
