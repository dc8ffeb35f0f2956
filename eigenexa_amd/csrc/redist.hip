// redist.hip -- the redistributions between the 2-D layouts of a solve, one all-to-all each (declared in eigx_context.h):
// bc_to_cyclic (a block-cyclic caller's blocks -> the cyclic layout the solvers work in) and cols_to_cyclic_dev (the
// eigenvector column blocks of the D&C and the back-transformation -> the caller's (block-)cyclic z).
#include "eigx_context.h"
#include "eigx_comm.h"
#include "../../include/eigenexa_amd.h"
#include <cstring>

namespace eigx {

namespace {

// local index l of process p (of P) -> global index, blocks of nb (nb = 1: cyclic, l*P + p)
__device__ __forceinline__ int bc_l2g(int l, int nb, int P, int p) { return ((l / nb) * P + p) * nb + l % nb; }

__device__ __host__ __forceinline__ int bc_owner(int g, int nb, int P) { return (g / nb) % P; }
__device__ __host__ __forceinline__ int bc_g2l(int g, int nb, int P) { return ((g / nb) / P) * nb + g % nb; }
// number of indices g < n that process p owns (NUMROC), usable on the device
__device__ __host__ __forceinline__ int bc_count(int n, int nb, int p, int P) {
  const int nblocks = n / nb;
  int cnt = (nblocks / P) * nb;
  const int extra = nblocks % P;
  if (p < extra) cnt += nb;
  else if (p == extra) cnt += n % nb;
  return cnt;
}

// Eigenvector column block of this rank (columns [c0, c0 + cnt), all n rows) -> pieces for the all-to-all that deals
// the matrix into the callers' 2-D (block-)cyclic blocks: the piece for rank (qx, qy) holds the rows that qx owns of
// those of my columns that qy owns: send[rank][ljr * nrmax + li]   (src/dc_redist1.F / dc_redist2.F play this role
// in the reference, between its D&C layout and the API layout)
__global__ void pack_z_pieces_kernel(const double* __restrict__ Z, int ldz, int n, int c0, int cnt, int nb, int Px, int Py,
                                     int row_major, int nrmax, size_t piece, double* __restrict__ send) {
  const int cl = blockIdx.y, qx = blockIdx.z;
  if (cl >= cnt) return;
  const int c = c0 + cl;
  const int qy = bc_owner(c, nb, Py);
  const int ljr = bc_g2l(c, nb, Py) - bc_count(c0, nb, qy, Py);
  const int dst = row_major ? qx * Py + qy : qx + qy * Px;
  const int nr = bc_count(n, nb, qx, Px);
  double* out = send + (size_t)dst * piece + (size_t)ljr * nrmax;
  const double* col = Z + (size_t)cl * ldz;
  for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < nr; li += gridDim.x * blockDim.x)
    out[li] = col[bc_l2g(li, nb, Px, qx)];
}
// z_user(li, lj) for my local columns that lie in source rank q's column range [q*zc, min((q+1)*zc, nvec))
__global__ void unpack_z_pieces_kernel(const double* __restrict__ recv, size_t piece, int nrmax, int nvec, int zc, int nb,
                                       int py, int Py, int nr, double* __restrict__ z, int ldz) {
  const int q = blockIdx.z;
  const int g0 = q * zc < nvec ? q * zc : nvec, g1 = (q + 1) * zc < nvec ? (q + 1) * zc : nvec;
  const int l0 = bc_count(g0, nb, py, Py), l1 = bc_count(g1, nb, py, Py);
  const int ljr = blockIdx.y;
  if (ljr >= l1 - l0) return;
  const double* src = recv + (size_t)q * piece + (size_t)ljr * nrmax;
  double* col = z + (size_t)(l0 + ljr) * ldz;
  for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < nr; li += gridDim.x * blockDim.x)
    col[li] = __hip_atomic_load(src + li, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- block-cyclic (nb x nb blocks, a ScaLAPACK descriptor's layout) -> cyclic, as one all-to-all ---------------------
// The element a rank holds at local (li, lj) is global (gi, gj) = (l2g(li), l2g(lj)); in the cyclic layout it belongs to
// rank (gi mod Px, gj mod Py) at local (gi div Px, gj div Py).  The piece for a destination is addressed by the RANK of
// the row / column among the sender's rows / columns that go to that destination: rrank[li], crank[lj] (host tables,
// O(n / P) integers); the receiver holds, for each of its cyclic rows / columns, the sender's grid coordinate and that
// rank (srcx / posr, srcy / posc).  This is what pdgemr2d does for the reference's callers (manual 3.4).
__global__ void bc_pack_kernel(const double* __restrict__ a, int lda, int nr, int nc, int nb, int Px, int px, int Py, int py,
                               int row_major, const int* __restrict__ rrank, const int* __restrict__ crank, int nrp,
                               size_t piece, double* __restrict__ send) {
  const int lj = blockIdx.y;
  if (lj >= nc) return;
  const int gj = bc_l2g(lj, nb, Py, py);
  const int qy = gj % Py;
  const int pc = crank[lj];
  for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < nr; li += gridDim.x * blockDim.x) {
    const int gi = bc_l2g(li, nb, Px, px);
    const int qx = gi % Px;
    const int dst = row_major ? qx * Py + qy : qx + qy * Px;
    send[(size_t)dst * piece + (size_t)pc * nrp + rrank[li]] = a[(size_t)lj * lda + li];
  }
}
__global__ void bc_unpack_kernel(const double* __restrict__ recv, size_t piece, int nrp, int clr, int clc, int Px, int Py,
                                 int row_major, const int* __restrict__ srcx, const int* __restrict__ posr,
                                 const int* __restrict__ srcy, const int* __restrict__ posc, double* __restrict__ out, int ldo) {
  const int lj = blockIdx.y;
  if (lj >= clc) return;
  const int sy = srcy[lj], pc = posc[lj];
  for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < clr; li += gridDim.x * blockDim.x) {
    const int sx = srcx[li];
    const int src = row_major ? sx * Py + sy : sx + sy * Px;
    out[(size_t)lj * ldo + li] = __hip_atomic_load(recv + (size_t)src * piece + (size_t)pc * nrp + posr[li], __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// one dimension of the index tables: n indices dealt in blocks of nb to P processes (me = p) -> cyclic over the same P
static void bc_tables_1d(int n, int nb, int P, int p, std::vector<int>& rank_of_local, std::vector<int>& src_of_cyc,
                         std::vector<int>& pos_of_cyc, int& max_piece) {
  const int nl = numroc(n, nb, p, P);
  rank_of_local.assign(nl > 0 ? nl : 1, 0);
  std::vector<int> cnt(P, 0);
  for (int l = 0; l < nl; ++l) {                       // my block-cyclic indices in ascending local order
    const int g = ((l / nb) * P + p) * nb + l % nb;
    rank_of_local[l] = cnt[g % P]++;
  }
  // what I receive as cyclic owner p: my cyclic index c is global g = c*P + p, held by block-cyclic process (g/nb) % P
  // at the rank it has among THAT process's indices going to me
  const int nc = local_count(n, P, p);
  src_of_cyc.assign(nc > 0 ? nc : 1, 0);
  pos_of_cyc.assign(nc > 0 ? nc : 1, 0);
  std::vector<int> seen(P, 0);
  for (int c = 0; c < nc; ++c) {                       // ascending global order = ascending local order on every sender
    const int g = c * P + p;
    const int s = (g / nb) % P;
    src_of_cyc[c] = s;
    pos_of_cyc[c] = seen[s]++;
  }
  max_piece = 0;
  for (int q = 0; q < P; ++q) { if (cnt[q] > max_piece) max_piece = cnt[q]; if (seen[q] > max_piece) max_piece = seen[q]; }
}

}  // namespace

int bc_to_cyclic(Context& ctx, const double* a, int lda, int n, int nb, double* out, int ldo, hipStream_t st) {
  const Grid& G = ctx.grid;
  const int P = G.nranks;
  std::vector<int> rrank, srcx, posr, crank, srcy, posc;
  int mr = 0, mc = 0;
  bc_tables_1d(n, nb, G.Px, G.px, rrank, srcx, posr, mr);
  bc_tables_1d(n, nb, G.Py, G.py, crank, srcy, posc, mc);
  // the piece extents must agree on every rank: an upper bound that depends on (n, nb, grid) only
  // (every block of a sender starts at the same residue mod P, so one destination can get ceil(nb/P) rows of EVERY block)
  const int nrp = (numroc(n, nb, 0, G.Px) / nb + 1) * ceil_div(nb, G.Px), ncp = (numroc(n, nb, 0, G.Py) / nb + 1) * ceil_div(nb, G.Py);
  if (mr > nrp || mc > ncp) {   // cannot happen (see the bound above); refuse rather than write past a piece
    fprintf(stderr, "[eigx] internal: block-cyclic piece bound violated (%d > %d or %d > %d)\n", mr, nrp, mc, ncp);
    return EIGX_ERR_INTERNAL;
  }
  const size_t piece = (size_t)nrp * ncp;
  const int nr = numroc(n, nb, G.px, G.Px), nc = numroc(n, nb, G.py, G.Py);
  const int clr = local_count(n, G.Px, G.px), clc = local_count(n, G.Py, G.py);
  const size_t nt = rrank.size() + srcx.size() + posr.size() + crank.size() + srcy.size() + posc.size();
  int* tab = ctx.pool.get_t<int>("mg.bctab", nt);
  int* htab = (int*)ctx.pool.get_host("mg.bctab", nt * sizeof(int));
  size_t o = 0;
  auto put = [&](const std::vector<int>& v) { int* d = tab + o; memcpy(htab + o, v.data(), v.size() * sizeof(int)); o += v.size(); return d; };
  const int* d_rrank = put(rrank); const int* d_srcx = put(srcx); const int* d_posr = put(posr);
  const int* d_crank = put(crank); const int* d_srcy = put(srcy); const int* d_posc = put(posc);
  EIGX_HIP_CHECK(hipMemcpyAsync(tab, htab, nt * sizeof(int), hipMemcpyHostToDevice, st));
  double* sendb = ctx.pool.get_t<double>("mg.xsend", piece * P);
  double* recvb = ctx.pool.get_t<double>("mg.xrecv", piece * P);
  if (nr > 0 && nc > 0)
    hipLaunchKernelGGL(bc_pack_kernel, dim3(8, nc), dim3(256), 0, st, a, lda, nr, nc, nb, G.Px, G.px, G.Py, G.py, G.row_major,
                       d_rrank, d_crank, nrp, piece, sendb);
  comm_exchange_big(ctx, COMM_WORLD, sendb, piece, recvb, piece, st);
  if (clr > 0 && clc > 0)
    hipLaunchKernelGGL(bc_unpack_kernel, dim3(8, clc), dim3(256), 0, st, (const double*)recvb, piece, nrp, clr, clc, G.Px,
                       G.Py, G.row_major, d_srcx, d_posr, d_srcy, d_posc, out, ldo);
  EIGX_HIP_CHECK(hipStreamSynchronize(st));   // the pinned table staging buffer is reused by the next call
  return EIGX_OK;
}

// Eigenvector column blocks (rank r holds columns [r zc, r zc + zc) of the first nvec, all n rows: zcols(ldz, zcnt) are
// mine, starting at global column zc0) -> the callers' 2-D (block-)cyclic blocks: one all-to-all of
// (rows of qx) x (my columns of qy) pieces.  Enqueued on st.  (eigen_h's split planes go through it one plane at a time.)
void cols_to_cyclic_dev(Context& ctx, int n, int nvec, int nb, int zc, int zc0, int zcnt, const double* zcols, int ldz,
                        double* z_user, int ldz_user, hipStream_t st) {
  const Grid& G = ctx.grid;
  const int P = G.nranks;
  const int nloc_r = numroc(n, nb, G.px, G.Px);
  const int nrmax = numroc(n, nb, 0, G.Px);
  const int ncmax = (zc / (nb * G.Py) + 2) * nb;
  const size_t piece = (size_t)nrmax * ncmax;
  double* sendb = ctx.pool.get_t<double>("mg.xsend", piece * P);
  double* recvb = ctx.pool.get_t<double>("mg.xrecv", piece * P);
  if (zcnt > 0)
    hipLaunchKernelGGL(pack_z_pieces_kernel, dim3(8, zcnt, G.Px), dim3(256), 0, st, zcols, ldz, n, zc0, zcnt, nb, G.Px,
                       G.Py, G.row_major, nrmax, piece, sendb);
  comm_exchange_big(ctx, COMM_WORLD, sendb, piece, recvb, piece, st);
  if (nloc_r > 0)
    hipLaunchKernelGGL(unpack_z_pieces_kernel, dim3(8, ncmax, P), dim3(256), 0, st, (const double*)recvb, piece, nrmax,
                       nvec, zc, nb, G.py, G.Py, nloc_r, z_user, ldz_user);
}

}  // namespace eigx
