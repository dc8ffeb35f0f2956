// zplanes.hip -- complex matrices as SPLIT PLANES: Re and Im as two real column-major arrays of one leading dimension, the
// form in which eigen_h (herm.hip), KMATH_EIGEN_HGEV (hgev.hip) and the complex triangular stages (ztri.hip) keep their
// O(n^3) work on the real fp64 MFMA GEMM.  What they share lives here (declared in one block of eigx_context.h):
//   zplanes          : both planes of a matrix in one pool buffer
//   zexpand / zsplit : interleaved complex(8) -> planes (the full Hermitian matrix from its upper triangle / a general block)
//   zjoin            : planes -> interleaved
//   zconj_transpose  : out = in^H
//   zgemm_planes     : C = alpha op(A) B + beta C as FOUR real products with beta accumulation
// The kernels are reached through these wrappers only; the wrappers choose the launch grids.  A block of the 2-D cyclic
// layout passes its Grid (global index = local index * P + p); one GPU passes none.
#include "eigx_context.h"

namespace eigx {

namespace {

// interleaved upper triangle of a -> planes of the full Hermitian matrix (lower = conj(upper), Im of the diagonal := 0).
// One 32 x 32 tile of the upper block triangle per workgroup; the mirrored tile goes through LDS, so both writes are
// coalesced.
__global__ __launch_bounds__(256) void hg_expand_kernel(const double* __restrict__ a, int lda, int n, double* __restrict__ Ar,
                                                        double* __restrict__ Ai, int ld) {
  __shared__ double sr[32][33], si[32][33];
  const int ti = blockIdx.x, tj = blockIdx.y;   // tile row, tile column
  if (ti > tj) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int i = ti * 32 + tx;
  for (int c = ty; c < 32; c += 8) {
    const int j = tj * 32 + c;
    double re = 0.0, im = 0.0;
    if (i <= j && j < n) {
      const size_t o = (size_t)i + (size_t)j * lda;
      re = a[2 * o];
      im = (i == j) ? 0.0 : a[2 * o + 1];
      Ar[(size_t)i + (size_t)j * ld] = re;
      Ai[(size_t)i + (size_t)j * ld] = im;
    }
    sr[c][tx] = re; si[c][tx] = im;   // element (ti*32 + tx, tj*32 + c)
  }
  __syncthreads();
  for (int c = ty; c < 32; c += 8) {
    const int r = tj * 32 + tx, col = ti * 32 + c;   // (r, col) = conj of (col, r) = sr[tx][c]
    if (r < n && col < r) {
      Ar[(size_t)r + (size_t)col * ld] = sr[tx][c];
      Ai[(size_t)r + (size_t)col * ld] = -si[tx][c];
    }
  }
}

// interleaved local block x (nr x nc) -> planes, column lc scaled by w[global column]^(-1/2) when w is given (F from U in
// one pass).  herm: x holds the upper triangle of a Hermitian matrix on the 2-D cyclic blocks -- entries below the global
// diagonal are not read (the planes keep what they hold there), Im of the diagonal := 0.
__global__ void hg_split_kernel(const double* __restrict__ x, int ldx, const double* __restrict__ w, int nr, int nc, int Px,
                                int px, int Py, int py, int herm, double* __restrict__ Pr, double* __restrict__ Pi, int ld) {
  for (int lc = blockIdx.y; lc < nc; lc += gridDim.y) {
    const int gc = lc * Py + py;
    const double s = w ? 1.0 / sqrt(w[gc]) : 1.0;
    for (int lr = blockIdx.x * blockDim.x + threadIdx.x; lr < nr; lr += gridDim.x * blockDim.x) {
      const int gr = lr * Px + px;
      if (herm && gr > gc) continue;
      const size_t o = (size_t)lr + (size_t)lc * ldx;
      const double re = x[2 * o];
      const double im = (herm && gr == gc) ? 0.0 : x[2 * o + 1];
      Pr[(size_t)lr + (size_t)lc * ld] = re * s;
      Pi[(size_t)lr + (size_t)lc * ld] = im * s;
    }
  }
}

// planes -> interleaved local block x (nr x nc); upper: only the entries on or above the global diagonal
__global__ void hg_join_kernel(const double* __restrict__ Pr, const double* __restrict__ Pi, int ld, int nr, int nc, int Px,
                               int px, int Py, int py, int upper, double* __restrict__ x, int ldx) {
  for (int lc = blockIdx.y; lc < nc; lc += gridDim.y) {
    const int gc = lc * Py + py;
    for (int lr = blockIdx.x * blockDim.x + threadIdx.x; lr < nr; lr += gridDim.x * blockDim.x) {
      if (upper && lr * Px + px > gc) continue;
      const size_t o = (size_t)lr + (size_t)lc * ldx;
      x[2 * o] = Pr[(size_t)lr + (size_t)lc * ld];
      x[2 * o + 1] = Pi[(size_t)lr + (size_t)lc * ld];
    }
  }
}

// out = in^H on planes (n x n)
__global__ __launch_bounds__(256) void zconj_transpose_kernel(const double* __restrict__ inr, const double* __restrict__ ini,
                                                              int ldi, double* __restrict__ outr, double* __restrict__ outi,
                                                              int ldo, int n) {
  __shared__ double Tr[32][33], Ti[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  for (int c = ty; c < 32; c += 8)
    if (r0 + tx < n && c0 + c < n) {
      Tr[c][tx] = inr[(size_t)(c0 + c) * ldi + r0 + tx];
      Ti[c][tx] = ini[(size_t)(c0 + c) * ldi + r0 + tx];
    }
  __syncthreads();
  for (int c = ty; c < 32; c += 8)
    if (c0 + tx < n && r0 + c < n) {
      outr[(size_t)(r0 + c) * ldo + c0 + tx] = Tr[tx][c];
      outi[(size_t)(r0 + c) * ldo + c0 + tx] = -Ti[tx][c];
    }
}

}  // namespace

ZPlanes zplanes(Context& ctx, const char* name, int ld, int ncols) {
  const size_t pl = (size_t)ld * (ncols > 0 ? ncols : 1);
  ZPlanes P;
  P.r = ctx.pool.get_t<double>(name, 2 * pl);
  P.i = P.r + pl;
  return P;
}

void zexpand(hipStream_t st, const double* a, int lda, int n, const ZPlanes& P, int ld) {
  const int nt = ceil_div(n, 32);
  hipLaunchKernelGGL(hg_expand_kernel, dim3(nt, nt), dim3(256), 0, st, a, lda, n, P.r, P.i, ld);
}

void zsplit(hipStream_t st, const double* x, int ldx, int nr, int nc, bool herm, const ZPlanes& P, int ld, const double* w,
            const Grid& G) {
  if (nr <= 0 || nc <= 0) return;
  hipLaunchKernelGGL(hg_split_kernel, zcol_grid(nr, nc), dim3(256), 0, st, x, ldx, w, nr, nc, G.Px, G.px, G.Py, G.py, herm ? 1 : 0,
                     P.r, P.i, ld);
}

void zjoin(hipStream_t st, const ZPlanes& P, int ld, int nr, int nc, bool upper, double* x, int ldx, const Grid& G) {
  if (nr <= 0 || nc <= 0) return;
  hipLaunchKernelGGL(hg_join_kernel, zcol_grid(nr, nc), dim3(256), 0, st, (const double*)P.r, (const double*)P.i, ld, nr, nc, G.Px,
                     G.px, G.Py, G.py, upper ? 1 : 0, x, ldx);
}

void zconj_transpose(hipStream_t st, int n, const ZPlanes& in, int ldi, const ZPlanes& out, int ldo) {
  const int t = ceil_div(n, 32);
  hipLaunchKernelGGL(zconj_transpose_kernel, dim3(t, t), dim3(256), 0, st, (const double*)in.r, (const double*)in.i, ldi, out.r,
                     out.i, ldo, n);
}

void zgemm_planes(hipStream_t st, char opA, int M, int N, int K, double alpha, const ZPlanes& A, int lda, const ZPlanes& B, int ldb,
                  double beta, const ZPlanes& C, int ldc, int tri_mode, const ZBatch& zb) {
  if (M <= 0 || N <= 0 || K <= 0) return;
  const char t = (opA == 'C') ? 'T' : 'N';
  const double sa = (opA == 'C') ? -1.0 : 1.0;   // sign of Ai under op
  auto one = [&](double al, const double* X, const double* Y, double be, double* Z) {
    dgemm_dev(st, t, 'N', M, N, K, al, X, lda, Y, ldb, be, Z, ldc, tri_mode, nullptr, nullptr, nullptr, zb.batch, zb.sA, zb.sB,
              zb.sC, zb.batch2, zb.sA2, zb.sB2, zb.sC2);
  };
  one(alpha, A.r, B.r, beta, C.r);            // Cr = op(Ar) Br - sa op(Ai) Bi
  one(-sa * alpha, A.i, B.i, 1.0, C.r);
  one(alpha, A.r, B.i, beta, C.i);            // Ci = op(Ar) Bi + sa op(Ai) Br
  one(sa * alpha, A.i, B.r, 1.0, C.i);
}

}  // namespace eigx
