// slk_als.hip -- implicit-feedback alternating least squares (Hu, Koren, Volinsky): slk_als_gram, slk_als_solve, slk_als_loss.
//
// A half-step fixes one table Y [n][D] and solves, for every row u of the other side with history N(u) and weights w = c - 1,
//     (G + lambda I + sum_{i in N(u)} w_ui y_i y_i^T) x_u = sum_{i in N(u)} (w_ui + 1) y_i,        G = Y^T Y,
// exactly, by Cholesky.  Rows do not interact: one unit owns one row from start to finish, builds the system on chip, factors
// it, substitutes twice and writes D floats.  Nothing passes between workgroups, no scratch in memory, no atomic but the counter
// of failed rows, no host wait.
//   k_als_gram / k_als_gram_reduce   G on the vector unit: a 256-thread workgroup stages 32 rows of Y in LDS and every thread
//                  keeps a T x T register tile of the D x D result; a workgroup walks a fixed set of row chunks and writes one
//                  partial tile, the partial tiles are added in workgroup order.  Which rows a workgroup takes depends on n
//                  alone, so two calls give the same bits, and G[i][j] and G[j][i] are the same chain with commuted factors:
//                  the result is symmetric bit for bit.
//   k_als_solve<DMAX, 64>    the light route: one wavefront (a 64-thread workgroup) per row
//   k_als_solve<DMAX, 256>   the workgroup route: 256 threads per row (long histories: the split rule for skewed lists)
// Both routes run the SAME arithmetic: every element of the system is a chain acc = fmaf(w y_i, y_j, acc) over the history in
// CSR order, every Cholesky update a chain over the columns in order, and only the thread that owns an element differs.  So a
// row's bits depend on its own CSR segment, Y, G and lambda -- not on the route ("als_wg_min_len"), the grid, the row list or
// who else is in the call.  Both kernels are launched for every call; the units whose row belongs to the other route leave at
// once (no host wait, no compaction pass), as in slk_foldin.hip.
//
// The system lives in LDS as the packed lower triangle of the AUGMENTED matrix [A; b^T] (D + 1 rows): carrying b as one more
// row through the right-looking factorization IS the forward substitution.  Column k is left unscaled (it holds L[i][k] * d_k,
// d_k = sqrt(pivot)); the scale 1 / d_k is applied where the column is read, which saves the barrier between scaling a column
// and using it: one barrier per column.
#include <float.h>

#include "slk_kernels.h"

#define SLK_ALS_MAX_DIM 128
#define SLK_ALS_WG_MIN_LEN 32       // "als_wg_min_len" 0 (automatic): histories from this length on take the workgroup route -- the
                                    // best sum of both half-steps among 8 / 16 / 32 / 64 / 256 / 1024 / 4096 / never on the Zipf shape
                                    // of scripts/bench_als.py (profiles/bench_als.json)
#define SLK_ALS_BATCH 16            // history rows the light route stages in LDS per trip (the workgroup route up to dim 64: four times as many)
#define SLK_ALS_GRAM_ROWS 32        // rows of the table a workgroup of k_als_gram stages per trip
#define SLK_ALS_GRAM_PART_ROWS 256  // a partial tile covers at least this many rows ...
#define SLK_ALS_GRAM_MAX_PARTS 1024 // ... and there are at most this many partial tiles

// ---- Gram matrix ----------------------------------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(256) void k_als_gram(const float *Y, int64_t n, int D, float *part) {
    constexpr int W = 16 * T;  // LDS row length (>= D), the tail zero
    constexpr int R = SLK_ALS_GRAM_ROWS;
    __shared__ float s_y[R * W];
    const int tj = (int)threadIdx.x & 15, ti = (int)threadIdx.x >> 4;
    float acc[T][T];
#pragma unroll
    for (int x = 0; x < T; ++x)
#pragma unroll
        for (int y = 0; y < T; ++y) acc[x][y] = 0.0f;
    const int64_t nchunks = (n + R - 1) / R;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t r0 = c * R;
        const int rows = n - r0 < R ? (int)(n - r0) : R;
        __syncthreads();  // the previous chunk is no longer read
        for (int e = (int)threadIdx.x; e < R * W; e += 256) {
            const int r = e / W, d = e % W;
            s_y[e] = (r < rows && d < D) ? Y[(size_t)(r0 + r) * D + d] : 0.0f;
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            float a[T], b[T];
#pragma unroll
            for (int x = 0; x < T; ++x) {
                a[x] = s_y[r * W + ti + 16 * x];
                b[x] = s_y[r * W + tj + 16 * x];
            }
#pragma unroll
            for (int x = 0; x < T; ++x)
#pragma unroll
                for (int y = 0; y < T; ++y) acc[x][y] = fmaf(a[x], b[y], acc[x][y]);
        }
    }
    float *out = part + (size_t)blockIdx.x * D * D;
#pragma unroll
    for (int x = 0; x < T; ++x)
#pragma unroll
        for (int y = 0; y < T; ++y) {
            const int i = ti + 16 * x, j = tj + 16 * y;
            if (i < D && j < D) out[i * D + j] = acc[x][y];
        }
}

// G[e] = the partial tiles' e-th elements, added in tile order: 64 elements per workgroup, the tiles in four contiguous
// slices summed side by side and then combined in slice order (a fixed association for a given number of tiles).
__global__ __launch_bounds__(256) void k_als_gram_reduce(const float *part, int nparts, int DD, float *G) {
    __shared__ float s_sum[256];
    const int el = (int)threadIdx.x & 63, slice = (int)threadIdx.x >> 6;
    const int e = (int)blockIdx.x * 64 + el;
    const int per = (nparts + 3) / 4;
    const int p0 = slice * per, p1 = p0 + per < nparts ? p0 + per : nparts;
    float s = 0.0f;
    if (e < DD)
        for (int p = p0; p < p1; ++p) s += part[(size_t)p * DD + e];
    s_sum[threadIdx.x] = s;
    __syncthreads();
    if (slice == 0 && e < DD) G[e] = ((s_sum[el] + s_sum[64 + el]) + s_sum[128 + el]) + s_sum[192 + el];
}

// ---- the half-step ----------------------------------------------------------------------------------------------------------------
struct slk_als_args {
    const float *Y;       // the fixed table
    const float *G;       // its Gram matrix [D][D]
    const int64_t *off, *cols;  // histories, CSR (rows: the side being solved, columns: rows of Y)
    const float *vals;    // c - 1 per entry
    const int64_t *rows;  // nullptr, or the row of unit r
    float *X;             // the table being solved
    double *loss;         // k_als_loss: one value per row
    int *fail;
    int64_t wg_min;       // histories of at least this many entries are the workgroup route's
    float lambda;
    int D;
};

// offset of row i in the packed lower triangle
__device__ __forceinline__ int slk_als_row(int i) { return i * (i + 1) / 2; }

template <int DMAX, int NT>
__global__ __launch_bounds__(NT) void k_als_solve(slk_als_args a) {
    constexpr int TY = NT / 8;  // threads are an 8-wide strip over the columns, TY rows deep
    // history rows staged per trip: a workgroup keeps more loads in flight (its histories are long; a row's bits do not depend
    // on where the batches are cut)
    constexpr int KB = (NT == 256 && DMAX <= 64) ? 4 * SLK_ALS_BATCH : SLK_ALS_BATCH;  // (dim > 64: the system fills the LDS budget)
    __shared__ float s_A[(DMAX + 1) * (DMAX + 2) / 2];
    __shared__ float s_y[KB * DMAX], s_wy[KB * DMAX];
    __shared__ int64_t s_id[KB];
    __shared__ float s_w[KB];
    __shared__ float s_inv[DMAX], s_x[DMAX];
    const int tid = (int)threadIdx.x;
    const int64_t u = a.rows ? a.rows[blockIdx.x] : (int64_t)blockIdx.x;
    const int64_t o0 = a.off[u];
    const int64_t m = a.off[u + 1] - o0;
    const int D = a.D;
    float *out = a.X + (size_t)u * D;
    if (m <= 0) {  // no history: the system's own solution is the zero row (the light route writes it)
        if (NT == 64)
            for (int d = tid; d < D; d += NT) out[d] = 0.0f;
        return;
    }
    if ((NT == 64) != (m < a.wg_min)) return;  // (the whole workgroup) the other route's
    const int tx = tid & 7, ty = tid >> 3;

    // 1. A = G + lambda I, b = 0
    for (int i = ty; i <= D; i += TY) {
        const int jm = i < D ? i : D - 1;
        for (int j = tx; j <= jm; j += 8) {
            float v = 0.0f;
            if (i < D) {
                v = a.G[i * D + j];
                if (i == j) v += a.lambda;
            }
            s_A[slk_als_row(i) + j] = v;
        }
    }
    // 2. the history, KB rows at a time: A[i][j] = fmaf(w y_i, y_j, A[i][j]), b[j] = fmaf(w + 1, y_j, b[j]), in CSR order
    for (int64_t k0 = 0; k0 < m; k0 += KB) {
        const int kb = m - k0 < KB ? (int)(m - k0) : KB;
        __syncthreads();  // the previous batch is no longer read
        if (tid < kb) {
            s_id[tid] = a.cols[o0 + k0 + tid];
            s_w[tid] = a.vals[o0 + k0 + tid];
        }
        __syncthreads();
        // half a wave per row, every load of the batch independent of the others (fixed trip counts: issued together)
#pragma unroll
        for (int it = 0; it < KB / (NT / 32); ++it) {
            const int kk = (tid >> 5) + it * (NT / 32);
            if (kk < kb) {
                const float w = s_w[kk];
                const float *y = a.Y + (size_t)s_id[kk] * D;
#pragma unroll
                for (int dd = 0; dd < DMAX / 32; ++dd) {
                    const int d = (tid & 31) + 32 * dd;
                    if (d < D) {
                        const float v = y[d];
                        s_y[kk * DMAX + d] = v;
                        s_wy[kk * DMAX + d] = w * v;
                    }
                }
            }
        }
        __syncthreads();
        for (int i = ty; i <= D; i += TY) {
            const int jm = i < D ? i : D - 1;
            for (int j = tx; j <= jm; j += 8) {
                float acc = s_A[slk_als_row(i) + j];
                if (i < D) {
                    for (int kk = 0; kk < kb; ++kk) acc = fmaf(s_wy[kk * DMAX + i], s_y[kk * DMAX + j], acc);
                } else {
                    for (int kk = 0; kk < kb; ++kk) acc = fmaf(s_w[kk] + 1.0f, s_y[kk * DMAX + j], acc);
                }
                s_A[slk_als_row(i) + j] = acc;
            }
        }
    }
    __syncthreads();
    // 3. right-looking Cholesky over the augmented matrix; every thread reads the same pivot, so the way out is uniform
    bool ok = true;
    for (int k = 0; k < D; ++k) {
        const float p = s_A[slk_als_row(k) + k];
        if (!(p > 0.0f && p <= FLT_MAX)) {
            ok = false;
            break;
        }
        const float inv = 1.0f / sqrtf(p);
        if (tid == 0) s_inv[k] = inv;
        for (int i = k + 1 + ty; i <= D; i += TY) {
            const float lik = s_A[slk_als_row(i) + k] * inv;
            const int jm = i < D ? i : D - 1;
            for (int j = k + 1 + tx; j <= jm; j += 8) {
                const float ljk = s_A[slk_als_row(j) + k] * inv;
                s_A[slk_als_row(i) + j] = fmaf(-lik, ljk, s_A[slk_als_row(i) + j]);
            }
        }
        __syncthreads();
    }
    if (!ok) {  // not positive definite in fp32 (or not finite): the row is left as it is and counted
        if (tid == 0) atomicAdd(a.fail, 1);
        return;
    }
    // 4. L^T x = z with the unscaled columns: x_i = (t_i / d_i) / d_i, then t_k -= A[i][k] x_i for k < i
    float *t = s_A + slk_als_row(D);
    for (int i = D - 1; i >= 0; --i) {
        const float inv = s_inv[i];
        const float xi = (t[i] * inv) * inv;
        for (int k = tid; k < i; k += NT) t[k] = fmaf(-s_A[slk_als_row(i) + k], xi, t[k]);
        if (tid == 0) s_x[i] = xi;
        __syncthreads();
    }
    for (int d = tid; d < D; d += NT) out[d] = s_x[d];
}

// ---- the objective, row by row ------------------------------------------------------------------------------------------------------
// x^T G x + sum_{i in N(u)} [c (1 - s)^2 - s^2] + lambda |x|^2, s = x . y_i: the sum over ALL items of c (p - s)^2 at the cost
// of the observed ones (the unobserved ones are s^2 each, together x^T G x minus the observed s^2).  Formed in float64 from
// the fp32 inputs; one wavefront per row, lane l takes entries l, l + 64, ... and columns l, l + 64 of G, the lanes' parts
// are added by a fixed tree.
template <int DMAX>
__global__ __launch_bounds__(64) void k_als_loss(slk_als_args a) {
    __shared__ float s_x[DMAX];
    __shared__ double s_red[64];
    const int tid = (int)threadIdx.x;
    const int64_t u = (int64_t)blockIdx.x;
    const int64_t o0 = a.off[u];
    const int64_t m = a.off[u + 1] - o0;
    const int D = a.D;
    for (int d = tid; d < D; d += 64) s_x[d] = a.X[(size_t)u * D + d];
    __syncthreads();
    double acc = 0.0;
    for (int j = tid; j < D; j += 64) {
        double col = 0.0;
        for (int i = 0; i < D; ++i) col = fma((double)a.G[i * D + j], (double)s_x[i], col);
        acc += (col + (double)a.lambda * (double)s_x[j]) * (double)s_x[j];
    }
    for (int64_t k = tid; k < m; k += 64) {
        const float *y = a.Y + (size_t)a.cols[o0 + k] * D;
        double s = 0.0;
        for (int d = 0; d < D; ++d) s = fma((double)s_x[d], (double)y[d], s);
        const double c = (double)a.vals[o0 + k] + 1.0;
        acc += c * (1.0 - s) * (1.0 - s) - s * s;
    }
    s_red[tid] = acc;
    __syncthreads();
    for (int o = 32; o >= 1; o >>= 1) {
        if (tid < o) s_red[tid] += s_red[tid + o];
        __syncthreads();
    }
    if (tid == 0) a.loss[u] = s_red[0];
}

// ---- entry points -----------------------------------------------------------------------------------------------------------------
static int als_check_dim(slk_ctx *ctx, const char *who, int64_t dim) {
    int vec, g;
    if (dim < 1 || dim > SLK_ALS_MAX_DIM || !slk_pick_layout((int)dim, &vec, &g))
        return slk_fail(ctx, SLK_EINVAL, "%s: embedding dim %lld unsupported (need dim %% 4 == 0 and <= %d, or dim <= 64)", who,
                        (long long)dim, SLK_ALS_MAX_DIM);
    return SLK_OK;
}

static int als_check_scope(slk_ctx *ctx, const char *who, const void *p0, const void *p1) {
    if (ctx->pp_active && ((p0 && p0 == ctx->pp_src_u) || (p1 && p1 == ctx->pp_src_u)))
        return slk_fail(ctx, SLK_EINVAL, "%s: the user rows of this table are ping-ponged (slk_user_pingpong_begin): the array holds "
                                         "only some of the current rows until slk_user_pingpong_end", who);
    return SLK_OK;
}

SLK_EXPORT int slk_als_gram(slk_ctx *ctx, const float *d_table, int64_t n_rows, int64_t dim, float *d_gram, void *stream) {
    if (!ctx) return SLK_EINVAL;
    int rc;
    if (n_rows < 0) return slk_fail(ctx, SLK_EINVAL, "slk_als_gram: n_rows %lld is negative", (long long)n_rows);
    if ((rc = als_check_dim(ctx, "slk_als_gram", dim))) return rc;
    if (!d_gram || (n_rows > 0 && !d_table)) return slk_fail(ctx, SLK_EINVAL, "slk_als_gram: d_table / d_gram is NULL");
    if ((rc = als_check_scope(ctx, "slk_als_gram", d_table, nullptr))) return rc;
    const int D = (int)dim, DD = D * D;
    const int64_t nchunks = (n_rows + SLK_ALS_GRAM_ROWS - 1) / SLK_ALS_GRAM_ROWS;
    const int64_t per = SLK_ALS_GRAM_PART_ROWS / SLK_ALS_GRAM_ROWS;
    int64_t nparts = (nchunks + per - 1) / per;
    if (nparts > SLK_ALS_GRAM_MAX_PARTS) nparts = SLK_ALS_GRAM_MAX_PARTS;
    slk_call call(ctx, stream);
    if ((rc = call.begin(SLK_K_SCORE))) return rc;
    if (nparts == 0) {
        SLK_HIP(ctx, hipMemsetAsync(d_gram, 0, (size_t)DD * sizeof(float), call.s));
        return SLK_OK;
    }
    if ((rc = slk_ensure(ctx, ctx->extra[AL_GPART], (size_t)nparts * DD * sizeof(float)))) return rc;
    float *part = (float *)ctx->extra[AL_GPART].p;
#define SLK_ALS_GRAM(T_) hipLaunchKernelGGL((k_als_gram<T_>), dim3((unsigned)nparts), dim3(256), 0, call.s, d_table, n_rows, D, part)
    switch ((D + 15) / 16) {
        case 1: SLK_ALS_GRAM(1); break;
        case 2: SLK_ALS_GRAM(2); break;
        case 3: SLK_ALS_GRAM(3); break;
        case 4: SLK_ALS_GRAM(4); break;
        case 5: SLK_ALS_GRAM(5); break;
        case 6: SLK_ALS_GRAM(6); break;
        case 7: SLK_ALS_GRAM(7); break;
        default: SLK_ALS_GRAM(8); break;
    }
#undef SLK_ALS_GRAM
    SLK_LAUNCH_CHECK(ctx, "k_als_gram");
    hipLaunchKernelGGL(k_als_gram_reduce, dim3((unsigned)((DD + 63) / 64)), dim3(256), 0, call.s, (const float *)part, (int)nparts, DD,
                       d_gram);
    SLK_LAUNCH_CHECK(ctx, "k_als_gram_reduce");
    return SLK_OK;
}

static int als_check_csr(slk_ctx *ctx, const char *who, int64_t n_rows, const int64_t *d_off, const int64_t *d_cols, const float *d_vals) {
    if (n_rows < 0 || n_rows > 0x7fffffff)
        return slk_fail(ctx, SLK_EINVAL, "%s: n_rows %lld must be in [0, 2^31)", who, (long long)n_rows);
    if (!d_off || !d_cols || !d_vals) return slk_fail(ctx, SLK_EINVAL, "%s: the histories (d_off / d_cols / d_vals) are NULL", who);
    return SLK_OK;
}

SLK_EXPORT int slk_als_solve(slk_ctx *ctx, const float *d_fixed, const float *d_gram, int64_t dim, float lambda, const int64_t *d_off,
                             const int64_t *d_cols, const float *d_vals, const int64_t *d_rows, int64_t n_rows, float *d_out,
                             int32_t *d_failed, void *stream) {
    if (!ctx) return SLK_EINVAL;
    int rc;
    if ((rc = als_check_csr(ctx, "slk_als_solve", n_rows, d_off, d_cols, d_vals))) return rc;
    if ((rc = als_check_dim(ctx, "slk_als_solve", dim))) return rc;
    if (!(lambda >= 0.0f && lambda <= FLT_MAX)) return slk_fail(ctx, SLK_EINVAL, "slk_als_solve: lambda %g must be finite and >= 0", (double)lambda);
    if (!d_fixed || !d_gram || !d_out || !d_failed)
        return slk_fail(ctx, SLK_EINVAL, "slk_als_solve: d_fixed / d_gram / d_out / d_failed is NULL");
    if ((rc = als_check_scope(ctx, "slk_als_solve", d_fixed, d_out))) return rc;
    if (n_rows == 0) return SLK_OK;
    slk_call call(ctx, stream);
    if ((rc = call.begin(SLK_K_USER_PASS))) return rc;
    slk_als_args a;
    memset(&a, 0, sizeof(a));
    a.Y = d_fixed;
    a.G = d_gram;
    a.off = d_off;
    a.cols = d_cols;
    a.vals = d_vals;
    a.rows = d_rows;
    a.X = d_out;
    a.fail = d_failed;
    a.wg_min = ctx->opt_als_wg_min_len > 0 ? ctx->opt_als_wg_min_len : SLK_ALS_WG_MIN_LEN;
    a.lambda = lambda;
    a.D = (int)dim;
    const dim3 grid((unsigned)n_rows);
    // long histories first: they are the launch's tail
#define SLK_ALS_SOLVE(DMAX_)                                                                  \
    do {                                                                                      \
        hipLaunchKernelGGL((k_als_solve<DMAX_, 256>), grid, dim3(256), 0, call.s, a);         \
        SLK_LAUNCH_CHECK(ctx, "k_als_solve (workgroup route)");                               \
        hipLaunchKernelGGL((k_als_solve<DMAX_, 64>), grid, dim3(64), 0, call.s, a);           \
        SLK_LAUNCH_CHECK(ctx, "k_als_solve (light route)");                                   \
    } while (0)
    if (dim <= 32) SLK_ALS_SOLVE(32);
    else if (dim <= 64) SLK_ALS_SOLVE(64);
    else SLK_ALS_SOLVE(128);
#undef SLK_ALS_SOLVE
    return SLK_OK;
}

SLK_EXPORT int slk_als_loss(slk_ctx *ctx, const float *d_rows_table, const float *d_fixed, const float *d_gram, int64_t dim, float lambda,
                            const int64_t *d_off, const int64_t *d_cols, const float *d_vals, int64_t n_rows, double *d_out,
                            void *stream) {
    if (!ctx) return SLK_EINVAL;
    int rc;
    if ((rc = als_check_csr(ctx, "slk_als_loss", n_rows, d_off, d_cols, d_vals))) return rc;
    if ((rc = als_check_dim(ctx, "slk_als_loss", dim))) return rc;
    if (!(lambda >= 0.0f && lambda <= FLT_MAX)) return slk_fail(ctx, SLK_EINVAL, "slk_als_loss: lambda %g must be finite and >= 0", (double)lambda);
    if (!d_rows_table || !d_fixed || !d_gram || !d_out)
        return slk_fail(ctx, SLK_EINVAL, "slk_als_loss: d_rows_table / d_fixed / d_gram / d_out is NULL");
    if ((rc = als_check_scope(ctx, "slk_als_loss", d_fixed, d_rows_table))) return rc;
    if (n_rows == 0) return SLK_OK;
    slk_call call(ctx, stream);
    if ((rc = call.begin(SLK_K_SCORE))) return rc;
    slk_als_args a;
    memset(&a, 0, sizeof(a));
    a.Y = d_fixed;
    a.G = d_gram;
    a.off = d_off;
    a.cols = d_cols;
    a.vals = d_vals;
    a.X = const_cast<float *>(d_rows_table);
    a.loss = d_out;
    a.lambda = lambda;
    a.D = (int)dim;
    const dim3 grid((unsigned)n_rows);
    if (dim <= 32) hipLaunchKernelGGL((k_als_loss<32>), grid, dim3(64), 0, call.s, a);
    else if (dim <= 64) hipLaunchKernelGGL((k_als_loss<64>), grid, dim3(64), 0, call.s, a);
    else hipLaunchKernelGGL((k_als_loss<128>), grid, dim3(64), 0, call.s, a);
    SLK_LAUNCH_CHECK(ctx, "k_als_loss");
    return SLK_OK;
}
