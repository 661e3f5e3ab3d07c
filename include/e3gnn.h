/*
 * e3gnn.h — C ABI of libe3gnn_hip.so, the MI355X (gfx950) implementation of the Scalable-E3-GNN
 * hot path.  Plain pointers and sizes only; no torch / C++ types cross this boundary.
 *
 * Every entry point returns an int status (E3_OK == 0); nothing throws across the ABI and nothing
 * allocates device memory behind the caller's back except the small per-plan tables created in
 * e3_l1tp_plan_create.  All kernels are enqueued on the caller's hipStream_t (passed as void*),
 * never synchronise, and are graph-capturable.
 *
 * Reference interface replaced (file:line in /root/reference/models/segnn/l1_tensor_prod.py):
 *   e3_l1tp_plan_create   <- L1TensorProduct.__init__ irreps partition, masks, counts   (:13-77)
 *   e3_l1tp_pack_weights  <- parameters + CG constants + norm buffers                   (:81-94,159-189)
 *   e3_l1tp_forward       <- L1TensorProduct.forward                                    (:234-299)
 *   e3_l1tp_backward      <- autograd of forward (reference relies on torch autograd)    (:234-299)
 * Builder-defined stages of the pipeline (no reference code in the mount) are
 * declared further below and say so.
 */
#ifndef E3GNN_H
#define E3GNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define E3GNN_ABI_VERSION 3

/* status codes */
enum {
  E3_OK = 0,
  E3_ERR_INVALID_ARG = 1,   /* null pointer, negative size, bad dtype ...                     */
  E3_ERR_BAD_IRREPS = 2,    /* l > 1, lmax != 1, parity not +-1, negative multiplicity          */
  E3_ERR_MISSING_WEIGHT = 3,/* an output class has columns but its weight pointer is NULL        */
  E3_ERR_UNSUPPORTED = 4,   /* shape exceeds what the kernels were built for                    */
  E3_ERR_HIP = 5,           /* a HIP runtime call failed; see e3_last_hip_error()              */
  E3_ERR_NO_DEVICE = 6
};

/* element types of in1 / in2 / weights / norms / out (all the same in one call) */
enum { E3_F32 = 0, E3_F64 = 1, E3_BF16 = 2 };

/* class index used for the 4-element pointer arrays below: l0e, l0o, l1e, l1o */
enum { E3_CLS_0E = 0, E3_CLS_0O = 1, E3_CLS_1E = 2, E3_CLS_1O = 3 };

typedef struct e3_l1tp_plan e3_l1tp_plan;

int         e3_abi_version(void);
const char* e3_status_string(int status);
const char* e3_last_hip_error(void);

/*
 * Plan = host+device description of one (in1_irreps -> out_irreps) tensor product with the fixed
 * second operand 1x0e+1x1o (spherical harmonics of an edge vector).
 * blocks: n x 3 int32, each (l, p, mul) with l in {0,1}, p in {+1,-1}, mul >= 0, in declaration
 * order (irreps are NOT sorted or merged: the column layout follows the declaration, :28-36,57-65).
 * Requires max l == 1 for both (the reference's asserts, :13-14).
 */
int e3_l1tp_plan_create(const int32_t* in1_blocks, int n_in1,
                        const int32_t* out_blocks, int n_out,
                        e3_l1tp_plan** plan);
int e3_l1tp_plan_destroy(e3_l1tp_plan* plan);

/* Shape queries (so a binding needs no second implementation of the bookkeeping). */
int e3_l1tp_in1_dim(const e3_l1tp_plan* plan);
int e3_l1tp_out_dim(const e3_l1tp_plan* plan);
/* rows/cols of weight matrix `cls` exactly as the reference allocates it (:81-88); 0,0 if absent */
int e3_l1tp_weight_shape(const e3_l1tp_plan* plan, int cls, int* rows, int* cols);
/* length of norm buffer `cls` (:159-162) */
int e3_l1tp_norm_len(const e3_l1tp_plan* plan, int cls);

/*
 * Packed weights: one device buffer holding the four weight matrices re-tiled for the MFMA
 * kernel (K padded per irreps block, 32-column tiles, CG constants 1/sqrt3, 1/sqrt6 folded in)
 * plus the per-output-column norm vector.  Size in bytes for a given dtype:
 */
int64_t e3_l1tp_packed_bytes(const e3_l1tp_plan* plan, int dtype);
/*
 * weights[cls], norms[cls]: device pointers of element type `dtype`, row-major contiguous, shapes
 * per e3_l1tp_weight_shape / e3_l1tp_norm_len.  weights[cls] may be NULL only when the class has
 * no output columns or no input rows.  norms may be NULL (module built without normalisation)
 * or hold NULL entries for empty classes.  `packed` must hold e3_l1tp_packed_bytes().
 */
int e3_l1tp_pack_weights(const e3_l1tp_plan* plan,
                         const void* const weights[4], const void* const norms[4],
                         int dtype, void* packed, void* stream);

/*
 * out[b, :] = L1TP(in1[b, :], in2[b, :])   for b in [0, B)
 *   in1 : [B, in1_dim]   row stride ld_in1 elements
 *   in2 : [B, 4] = [Y0, Y1x, Y1y, Y1z], row stride ld_in2 elements; ld_in2 == 0 broadcasts row 0
 *   out : [B, out_dim]   row stride ld_out; every column is written
 * `kernel`: 0 = auto, 1 = force the generic kernel, 2 = force the MFMA kernel (E3_ERR_UNSUPPORTED
 * if the plan / dtype cannot use it).
 */
int e3_l1tp_forward(const e3_l1tp_plan* plan,
                    const void* in1, int64_t ld_in1,
                    const void* in2, int64_t ld_in2,
                    const void* packed,
                    void* out, int64_t ld_out,
                    int64_t B, int dtype, int kernel, void* stream);

/*
 * Gradients of sum(out * grad_out).  grad_in1 [B,in1_dim] and grad_in2 [B,4] are overwritten;
 * grad_weights[cls] (same shapes as weights) are overwritten.  When in2 was broadcast
 * (ld_in2 == 0) grad_in2 is a single row [1,4].  `workspace` must hold
 * e3_l1tp_backward_workspace_bytes() bytes.  Any of grad_in1 / grad_in2 / grad_weights may be
 * NULL to skip that gradient.  grad_out has row stride ld_gout >= out_dim, grad_in1 row stride
 * ld_gin1 >= in1_dim; grad_in2 is contiguous.  As in e3_l1tp_forward, a leading dimension below
 * the row width, or ld_in2 in {1, 2, 3}, is E3_ERR_INVALID_ARG before any launch.
 */
int64_t e3_l1tp_backward_workspace_bytes(const e3_l1tp_plan* plan, int64_t B, int dtype);
int e3_l1tp_backward(const e3_l1tp_plan* plan,
                     const void* in1, int64_t ld_in1,
                     const void* in2, int64_t ld_in2,
                     const void* const weights[4], const void* const norms[4],
                     const void* grad_out, int64_t ld_gout,
                     void* grad_in1, int64_t ld_gin1,
                     void* grad_in2,
                     void* const grad_weights[4],
                     void* workspace,
                     int64_t B, int dtype, void* stream);

/* =================================================================================================
 * Radius graph (builder-defined: the reference mount has no graph code; the spec
 * below is this repo's contract and oracle/radius_graph_oracle.c is its CPU statement).
 *
 *   grid   : per axis a,  n_a = clamp(floor((hi_a-lo_a) / (r*1.0001f)), 1, 256)   (fp32 arithmetic)
 *            cell c_a(p) = clamp((int)floorf((p_a-lo_a) * (n_a/(hi_a-lo_a))), 0, n_a-1)
 *   key    : 30-bit Morton interleave of (cx,cy,cz) (x lowest bit)
 *   order  : stable sort by key; new id = rank; perm[new] = old
 *   edge   : (src=j -> dst=i), i != j, iff d2 <= fl32(r*r) with
 *            d2 = fl32(fl32(fl32(dx*dx)+fl32(dy*dy))+fl32(dz*dz)), dx = fl32(x_i-x_j) (no FMA contraction)
 *   output : CSR by dst in NEW ids: rowptr[N+1] (int32), src[E] (int32) ascending inside each row.
 * All integer outputs are bit-exact functions of the inputs.
 *
 * Call sequence (sizes are only known after the count pass, so the caller allocates `src`):
 *   e3_rg_workspace_bytes -> e3_rg_sort_count (fills perm, sorted_pos4, rowptr) -> read E = rowptr[N]
 *   -> e3_rg_fill (fills src).
 * ================================================================================================= */
typedef struct e3_rg_params {
  float lo[3], hi[3];
  float r;
  int32_t n[3];   /* filled by e3_rg_grid */
  float inv[3];   /* filled by e3_rg_grid */
  int32_t bits;   /* filled by e3_rg_grid: Morton bits per axis */
} e3_rg_params;

int     e3_rg_grid(e3_rg_params* prm);                     /* host only: derives n, inv, bits from lo/hi/r */
int64_t e3_rg_workspace_bytes(int64_t N, const e3_rg_params* prm);
/* pos [N,3] fp32 contiguous (device). Outputs (device): perm [N] int32, sorted_pos4 [N,4] fp32
 * (x,y,z,0 in new order), rowptr [N+1] int32. */
int e3_rg_sort_count(const float* pos, int64_t N, const e3_rg_params* prm,
                     int32_t* perm, float* sorted_pos4, int32_t* rowptr,
                     void* workspace, int64_t workspace_bytes, void* stream);
/* src [E] int32 (device), E = rowptr[N]; must follow e3_rg_sort_count with the same workspace. */
int e3_rg_fill(int64_t N, const e3_rg_params* prm, const float* sorted_pos4, const int32_t* rowptr,
               int32_t* src, void* workspace, int64_t workspace_bytes, void* stream);

/* Orthorhombic periodic box, chosen per axis: `periodic` bit a (0..2) = axis a periodic, the other axes open as above.
 * Same grid, workspace, call sequence and outputs as e3_rg_sort_count / e3_rg_fill; on a periodic axis a, with
 * L = fl32(hi_a - lo_a), invL = fl32(1 / L), hL = fl32(0.5 * L):
 *   wrap   : w = fl32(p - fl32(L * floorf(fl32(fl32(p - lo_a) * invL)))); then one correction step:
 *            w >= hi_a -> w = fl32(w - L), else w < lo_a -> w = fl32(w + L).  Cell and key are taken from w, and
 *            sorted_pos4 holds w (open axes: p unchanged).
 *   cells  : the 27 neighbour cells are taken modulo n_a (a cell named twice, n_a <= 2, is scanned once).
 *   edge   : dx = fl32(x_i - x_j); dx > hL -> dx = fl32(dx - L), else dx < -hL -> dx = fl32(dx + L)  (x_i, x_j wrapped);
 *            then d2 and the test d2 <= fl32(r*r) exactly as in the open box.
 * Requires 0 < L and 2 r < L on every periodic axis (the minimum image is then unique: no pair has two edges, no
 * particle is its own neighbour); otherwise, or periodic outside [0, 7], E3_ERR_INVALID_ARG before any launch.
 * `periodic` must be the same in both calls. */
int e3_rg_sort_count_pbc(const float* pos, int64_t N, const e3_rg_params* prm, int32_t periodic,
                         int32_t* perm, float* sorted_pos4, int32_t* rowptr,
                         void* workspace, int64_t workspace_bytes, void* stream);
int e3_rg_fill_pbc(int64_t N, const e3_rg_params* prm, int32_t periodic, const float* sorted_pos4,
                   const int32_t* rowptr, int32_t* src, void* workspace, int64_t workspace_bytes, void* stream);

/* General (triclinic) periodic cell, periodic on all three lattice directions: the *_cell entries of the graph builder, the
 * geometry, its backward, the strained pair and e3_msg_forward.  cell[9] (host fp32, row-major) holds the lattice vectors as
 * rows, a_a = cell[3 a .. 3 a + 2] (the ASE convention); origin[3] (host fp32) is the corner the cell is spanned from.
 * Derived on the host in fp64 from the fp32 entries and rounded once to fp32 (e3_cell_derive returns them):
 *   G = cell^-1 (cofactors over the determinant), so the fractional coordinate is s = (p - origin) G;
 *   heights h_a = 1 / |G[:, a]| (the distance between the two faces that a_a joins);  V = |det cell|.
 * Every fp32 operation below is rounded on its own (no FMA contraction):
 *   frac(v)_a   = fl(fl(fl(v_0 G[0,a]) + fl(v_1 G[1,a])) + fl(v_2 G[2,a]))
 *   shift(v, n) : v_c <- fl(v_c - fl(fl(fl(n_0 cell[0,c]) + fl(n_1 cell[1,c])) + fl(n_2 cell[2,c])))
 *   wrap   : s = frac(fl(p - origin)); w = shift(p, floorf(s)); then ONE correction step: s' = frac(fl(w - origin)) and, for
 *            a = 0, 1, 2 in turn, s'_a >= 1 -> w = fl(w - a_a), else s'_a < 0 -> w = fl(w + a_a).  sorted_pos4 holds the
 *            Cartesian w.
 *   grid   : the open grid (e3_rg_grid, cell_of, Morton key above) of the points q_a = fl(frac(fl(w - origin))_a h_a) in the
 *            box lo = 0, hi = h: n_a = clamp(floor(h_a / (r 1.0001f)), 1, 256).  prm is what e3_rg_grid makes of
 *            lo = (0,0,0), hi = (h_0,h_1,h_2) and r; workspace, sort and call sequence are those of e3_rg_sort_count.
 *   cells  : the 27 neighbour cells modulo n_a in every direction (a cell named twice, n_a <= 2, is scanned once).  q_a is
 *            the coordinate along the unit normal of the faces of direction a, so a pair with |d| <= r has
 *            |dq_a| <= r (modulo h_a) and lies at most one grid cell apart when the rounding of q is below half of the
 *            1e-4 r margin of the cell width.  q carries 3 roundings of s and one of the product:
 *            |err q_a| <= 2^-22 h_a K_a, K_a = sum_c |p_c - origin_c| |G[c,a]| (K_a = s_a <= 1 in an orthorhombic cell,
 *            and at most the sum of the |s_b| |a_b| / h_a of a wrapped point in a skewed one), i.e. the bound holds for
 *            r / h_a >= 2^-7 K_a at least (2 * 2^-22 K_a h_a <= 1e-4 r) -- the order of the n_a <= 256 clamp of the grid.
 *   edge   : d = fl(x_i - x_j) on wrapped positions; in the cells whose 3x3x3 neighbourhood crosses a face of the grid, and
 *            everywhere when some n_a < 5: d = shift(d, rintf(frac(d))) (elsewhere rintf(frac(d)) = 0: the shift is the
 *            identity); then d2 and the test d2 <= fl(r*r) exactly as in the open box.
 *   rel    : the edge vector of the geometry, message and backward kernels: d = fl(x_src - x_dst), rel = shift(d,
 *            rintf(frac(d))) -- valid for wrapped and for unwrapped coordinates (positions moved by whole lattice vectors).
 *            The shift is constant, so the backward is the open backward at rel.
 * Requires finite entries, a non-singular cell and 0 < 2 r < min_a h_a (fp32 compare): the image of a pair with |d| <= r is
 * then unique and is the one with every |ds_a| < 1/2, which rintf finds; for wrapped points n is in {-1,0,1}^3.  Otherwise
 * E3_ERR_INVALID_ARG before any launch (the geometry and message entries have no cutoff: they check the cell alone).
 * e3_rg_sort_count_cell also rejects a prm whose lo / hi are not 0 / the heights.  cell and origin must be the same in both
 * calls of the builder.  Strain: r' = (I + eps_s) rel exactly as in e3_edge_geometry_strained; stress = (1/V) dE/deps. */
int e3_cell_derive(const float cell[9], float ginv[9], float heights[3], float* volume);  /* host only */
int e3_rg_sort_count_cell(const float* pos, int64_t N, const e3_rg_params* prm, const float cell[9], const float origin[3],
                          int32_t* perm, float* sorted_pos4, int32_t* rowptr,
                          void* workspace, int64_t workspace_bytes, void* stream);
int e3_rg_fill_cell(int64_t N, const e3_rg_params* prm, const float cell[9], const float origin[3],
                    const float* sorted_pos4, const int32_t* rowptr, int32_t* src,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* Capped rows: per node the k nearest neighbours inside r, k in [1, 64] (radius_graph(..., max_neighbors=k)).  Everything up
 * to the edge test is the uncapped builder of the mode: wrapping, grid, Morton order, perm, sorted_pos4 and the edge test with
 * its explicitly rounded d2 (and image shift).  Call the sources that pass the test for row i its full neighbourhood, of
 * size deg_i (what the count pass counts).
 *   deg_i <= k : the row is the uncapped row: the same ids in the same order.
 *   deg_i >  k : the row keeps the k sources with the smallest key (d2, j): d2 is the fp32 value the edge test computed for
 *                the pair (the same bits, image shift included), j the source's new (Morton) id; d2 is compared first, ties
 *                on d2 go to the lower j.  The kept ids are written in ascending j, as in every other row.
 *   rowptr     : the exclusive scan of min(deg_i, k).
 * All integer outputs stay bit-exact functions of the inputs.  The capped graph is DIRECTED: j -> i can exist without
 * i -> j (j among the k nearest of i does not make i one of the k nearest of j).
 *
 * Call sequence: e3_rg_sort_count* (unchanged: rowptr_full, and the full degrees stay in the workspace)
 *   -> e3_rg_cap_rowptr (rowptr_capped, stats) -> read E = rowptr_capped[N] and stats -> e3_rg_fill_nearest* (fills src)
 * on the same stream, with the same prm / periodic / cell and the same workspace in the first and the last call.
 *
 * e3_rg_cap_rowptr: deg_i is the WRAPPING int32 difference rowptr_full[i + 1] - rowptr_full[i] (each degree is below 2^31
 * even when the running sum has wrapped, i.e. when the uncapped graph does not fit int32).  rowptr_capped [N+1] may be the
 * buffer of rowptr_full (every degree is read before the first entry is written).  stats (device, 2 x int64): the number of
 * rows with deg_i > k, and the full edge count sum deg_i in 64 bits.  workspace: e3_rg_cap_workspace_bytes(N) bytes of its
 * own (the capped degrees and the scan's temporary storage; NOT the builder's workspace, whose contents the fill still needs).
 * e3_rg_fill_nearest*: src [E] int32.  One wave per non-empty cell, as the plain fill; a row above k keeps a sorted best-k
 * across the wave and merges batches of 64 candidates into it; a neighbourhood of more than 1024 candidates arrives in
 * several chunks, between which such a row parks its best ids in its own k slots of src.  No scratch beyond the builder's
 * workspace.  k outside [1, 64] or a NULL pointer: E3_ERR_INVALID_ARG before any launch. */
int64_t e3_rg_cap_workspace_bytes(int64_t N);
int e3_rg_cap_rowptr(const int32_t* rowptr_full, int64_t N, int k, int32_t* rowptr_capped, int64_t* stats,
                     void* workspace, int64_t workspace_bytes, void* stream);
int e3_rg_fill_nearest(int64_t N, const e3_rg_params* prm, const float* sorted_pos4, const int32_t* rowptr_capped, int k,
                       int32_t* src, void* workspace, int64_t workspace_bytes, void* stream);
int e3_rg_fill_nearest_pbc(int64_t N, const e3_rg_params* prm, int32_t periodic, const float* sorted_pos4,
                           const int32_t* rowptr_capped, int k, int32_t* src,
                           void* workspace, int64_t workspace_bytes, void* stream);
int e3_rg_fill_nearest_cell(int64_t N, const e3_rg_params* prm, const float cell[9], const float origin[3],
                            const float* sorted_pos4, const int32_t* rowptr_capped, int k, int32_t* src,
                            void* workspace, int64_t workspace_bytes, void* stream);

/* =================================================================================================
 * Edge / node stages of the SEGNN forward around the tensor product (builder-defined, SURVEY.md
 * §8a-N2, N3; fp32).  Graph = CSR by dst from e3_rg_* (rowptr [N+1], src [E], positions pos4 [N,4]).
 *   rel_e  = x[src_e] - x[dst_e];  d_e = |rel_e|
 *   Y_e    = [1, sqrt(3) rel_e/d_e]   ("component" normalised real SH, l<=1, xyz order; Y1 = 0 if d_e = 0)
 *   A_i    = [1, mean_{e -> i} Y1_e]  (node attribute; [1,0,0,0] for isolated nodes)
 * ================================================================================================= */
/* edge_y [E,4], edge_d [E] (may be NULL), node_a [N,4] (may be NULL) */
int e3_edge_geometry(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N,
                     float* edge_y, float* edge_d, float* node_a, void* stream);
/* Periodic box (the *_pbc entries of the geometry, its backward and e3_msg_forward): box[3] (host) = L_a per axis, 0 = open
 * axis.  rel_e is the minimum image of x[src_e] - x[dst_e], per periodic axis
 *   d = fl32(x_src - x_dst);  rel = fl32(d - fl32(L * rintf(fl32(d * invL)))),   invL = fl32(1 / L)
 * which holds for wrapped and for unwrapped coordinates (positions shifted by whole periods).  The shift is constant, so
 * the backward is the open-box backward at the shifted vector.  A negative or non-finite L is E3_ERR_INVALID_ARG. */
int e3_edge_geometry_pbc(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, const float box[3],
                         float* edge_y, float* edge_d, float* node_a, void* stream);
/* general cell (cell[9] as in e3_rg_sort_count_cell): rel_e = the minimum image defined there */
int e3_edge_geometry_cell(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, const float cell[9],
                          float* edge_y, float* edge_d, float* node_a, void* stream);
/* out[e] = [ h[dst_e] (D) | h[src_e] (D) | extra[e] (n_extra, may be 0) ]   row strides in elements */
int e3_gather_concat(const float* h, int64_t ld_h, int D, const int32_t* rowptr, const int32_t* src, int64_t N,
                     const float* extra, int n_extra, float* out, int64_t ld_out, void* stream);
/* gate: in = [ns scalars | nv gate scalars | nv vectors (xyz adjacent)] -> out = [silu(s) | sigmoid(g)*v] */
int e3_gate(const float* in, int64_t ld_in, float* out, int64_t ld_out, int64_t B, int ns, int nv, void* stream);
/* agg[i] = sum over row i of msg[e] (fixed edge order => bitwise reproducible); D columns */
int e3_segment_sum(const float* msg, int64_t ld_msg, const int32_t* rowptr, int64_t N, int D,
                   float* agg, int64_t ld_agg, void* stream);

/* Sharded graph (sharding.GridHalo.split_graph): from the CSR graph of the local cloud (owned + ghost rows) and the per-row
 * ghost flags (uint8), drop the edges INTO ghost rows and split the rest by the ownership of their src -- classification and
 * compaction in one call, every output sorted by dst:
 *   rowptr_kept [N+1], (src_kept, dst_kept) [E_kept]: the graph without the dropped rows' edges
 *   (src_interior, dst_interior): kept edges with an owned src;  (src_boundary, dst_boundary): kept edges with a ghost src
 *   counts[0..2] = E_kept, E_interior, E_boundary (device memory; the caller reads them once to size its views)
 * The six edge outputs need room for E elements each; workspace = e3_split_edges_workspace_bytes(N) bytes. */
int64_t e3_split_edges_workspace_bytes(int64_t N);
int e3_split_edges(const int32_t* rowptr, const int32_t* src, const uint8_t* is_ghost, int64_t N, int64_t E,
                   int32_t* rowptr_kept, int32_t* src_kept, int32_t* dst_kept, int32_t* src_interior, int32_t* dst_interior,
                   int32_t* src_boundary, int32_t* dst_boundary, int32_t* counts, void* workspace, void* stream);

/* Periodic halo (sharding.GridHalo with `periodic`): wrap the owned positions and pick the particles each ghost image
 * needs -- a two-call pair in the style of e3_rg_sort_count / e3_rg_fill.
 *   wrap   : on the axes of `periodic` (bits 0..2) with the domain lo[3] / hi[3] (host fp32): exactly the wrap of
 *            e3_rg_sort_count_pbc (L = fl32(hi_a - lo_a), invL = fl32(1 / L)); open axes unchanged -> pos_wrapped [n,3].
 *   entry  : entries[e] (host, n_entries <= 26) = {lo[3], hi[3], shift[3]} fp32; particle i is in entry e iff
 *            lo[a] <= w_i[a] < hi[a] on every axis (fp32 compares of the wrapped position).
 *   output : idx [total] int32 and ghost_pos [total,3] = fl32(pos_wrapped[idx] + shift), grouped by entry, ascending particle
 *            ids inside a group (the order of nonzero() on an entry-major [n_entries, n] mask); counts[e] (device) = the
 *            size of group e, total = sum of counts.
 * Call sequence: e3_halo_select_workspace_bytes -> e3_halo_select_count (pos_wrapped, counts) -> read counts
 *   -> e3_halo_select_fill (idx, ghost_pos; the same workspace, entries and wrap arguments, `total` = the capacity of idx).
 * E3_ERR_INVALID_ARG before any launch for n_entries outside [0, 26], a non-finite or empty lo / hi, periodic outside [0, 7],
 * 2 r >= L on a periodic axis, a NaN entry bound or a non-finite shift, or n * n_entries >= 2^31 - 1. */
#define E3_HALO_MAX_ENTRIES 26
typedef struct e3_halo_entry {
  float lo[3], hi[3], shift[3];
} e3_halo_entry;
int64_t e3_halo_select_workspace_bytes(int64_t n, int n_entries);
int e3_halo_select_count(const float* pos, int64_t n, const float lo[3], const float hi[3], int32_t periodic, float r,
                         const e3_halo_entry* entries, int n_entries, float* pos_wrapped, int32_t* counts, void* workspace,
                         int64_t workspace_bytes, void* stream);
int e3_halo_select_fill(const float* pos_wrapped, int64_t n, const float lo[3], const float hi[3], int32_t periodic, float r,
                        const e3_halo_entry* entries, int n_entries, int64_t total, int32_t* idx, float* ghost_pos,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* Morton-range halo (sharding.MortonPartition / MortonHalo): equal-COUNT ownership of a non-uniform cloud, open boxes only.
 *   grid   : the domain lo[3] / hi[3] (host fp32) cut into n_cells[a] cells per axis, each a power of two in [1, 128];
 *            cell and key of a position exactly as in e3_rg_sort_count: c_a = clamp(floorf(fl32(fl32(p_a - lo_a) * inv_a)),
 *            0, n_a - 1), inv_a = fl32(n_a / fl32(hi_a - lo_a)), key = Morton interleave of (cx, cy, cz), x lowest bit.
 *   keys   : e3_morton_keys writes key_i (int32) of every position: the input of the partition's histogram.
 *   owner  : splitters[n_ranks + 1] (host int32, non-decreasing, splitters[0] = 0): rank q owns the cells with
 *            splitters[q] <= key < splitters[q + 1]; equal neighbours = a rank that owns nothing; a key at or beyond the
 *            last splitter belongs to the last rank.
 *   select : particle i (owned by self_rank) goes to rank q != self_rank iff q owns at least one cell (x, y, z) with
 *            cell(fl32(p_a - r)) <= c_a <= cell(fl32(p_a + r)) on every axis.  Cells are at least r wide, so these are at
 *            most 3 (4 under adverse rounding of p +- r) cells per axis, and rounding is monotone: every p' with
 *            |p'_a - p_a| <= r on every axis lies in one of them, whatever fp32 does to p +- r.
 *   output : idx [total] int32, grouped by destination rank ascending, ascending particle ids inside a group (the order of
 *            nonzero() on a rank-major [n_ranks, n] mask); counts[q] (device, n_ranks values, counts[self_rank] = 0) = the
 *            size of group q, total = sum of counts.
 * Call sequence: e3_morton_select_workspace_bytes -> e3_morton_select_count (counts) -> read counts -> e3_morton_select_fill
 *   (idx; the same workspace, grid, splitters and r; `total` = the capacity of idx).
 * E3_ERR_INVALID_ARG before any launch (and before any HIP call) for n_ranks outside [1, 64], self_rank outside the ranks,
 * splitters that decrease or do not start at 0, n_cells not powers of two in [1, 128], a cell narrower than r on an axis with
 * more than one cell (fl32(hi_a - lo_a) / n_a < r; a single cell is selected whatever r is), r <= 0 or non-finite, a non-finite or empty box, or n * n_ranks >= 2^31 - 1. */
#define E3_MORTON_MAX_RANKS 64
int e3_morton_keys(const float* pos, int64_t n, const float lo[3], const float hi[3], const int32_t n_cells[3], int32_t* keys,
                   void* stream);
int64_t e3_morton_select_workspace_bytes(int64_t n, int n_ranks);
int e3_morton_select_count(const float* pos, int64_t n, const float lo[3], const float hi[3], const int32_t n_cells[3], float r,
                           const int32_t* splitters, int n_ranks, int self_rank, int32_t* counts, void* workspace,
                           int64_t workspace_bytes, void* stream);
int e3_morton_select_fill(const float* pos, int64_t n, const float lo[3], const float hi[3], const int32_t n_cells[3], float r,
                          const int32_t* splitters, int n_ranks, int self_rank, int64_t total, int32_t* idx, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* Migration of particles between ranks (sharding.Halo.migrate): split the rows of a row table by a GIVEN owner.
 *   table  : int32 [n, W], row-major: whatever the caller keeps per particle, viewed as 32-bit words (sharding.pack_rows).
 *   owner  : int32 [n] (device): the rank each row belongs to now.  An input -- the ownership rule is halo.owner_of and
 *            nothing here restates it.  A row whose owner lies outside [0, n_ranks) is INVALID: it is counted, never
 *            copied, and nothing is indexed by its owner.
 *   count  : counts [n_ranks + 1] (device): counts[q] = the rows with owner == q (counts[self_rank] = the stayers),
 *            counts[n_ranks] = the invalid rows; the sum is n.
 *   output : stay [counts[self_rank], W] = the rows with owner == self_rank in their original order; send [.., W] = the
 *            valid rows with owner != self_rank, grouped by destination rank ascending, ascending row ids inside a group.
 *            Plain stores in a fixed order: the same inputs give the same bytes.  Rows past the counts are not written.
 * Call sequence: e3_migrate_workspace_bytes -> e3_migrate_count (counts) -> read counts -> e3_migrate_fill (the same
 *   workspace, owner, n_ranks and self_rank; `counts` = the HOST copy of what was read; stay_rows / send_rows = the
 *   capacities of stay / send in rows).
 * E3_ERR_INVALID_ARG before any launch (and before any HIP call) for n_ranks outside [1, E3_MORTON_MAX_RANKS], self_rank
 * outside the ranks, n < 0, n * n_ranks >= 2^31 - 1, a NULL pointer that would be used, a workspace too small; fill also
 * for W outside [1, 4096], n * W >= 2^31 - 1, a negative count, counts that do not sum to n, and stay_rows / send_rows
 * smaller than the counts imply.  n = 0 is legal: count zeroes the counts, fill launches nothing. */
int64_t e3_migrate_workspace_bytes(int64_t n, int n_ranks);
int e3_migrate_count(const int32_t* owner, int64_t n, int n_ranks, int self_rank, int32_t* counts, void* workspace,
                     int64_t workspace_bytes, void* stream);
int e3_migrate_fill(const int32_t* table, const int32_t* owner, int64_t n, int W, int n_ranks, int self_rank,
                    const int32_t* counts, int64_t stay_rows, int64_t send_rows, int32_t* stay, int32_t* send, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* =================================================================================================
 * General SH tensor product, l <= 2 (builder-defined generalisation of the reference operator, which
 * hard-asserts lmax == 1, l1_tensor_prod.py:13-14).
 *
 *   in1  : irreps blocks (l, p, mul), l in {0,1,2}, declaration order = column order (m fastest)
 *   in2  : real "component" spherical harmonics up to lmax_sh in {1,2}: [Y0 | Y1 xyz | Y2 (5)]
 *   out[c3, w, m3] = norm * sum_{paths (l1,l2) -> c3} sum_k W_c3[row(path,k), w]
 *                           sum_{m1,m2} C^{l1 l2 l3}[m1,m2,m3] in1[c1,k,m1] in2[l2,m2]
 *   classes c = 2*l + (p == -1 ? 1 : 0)  (0e,0o,1e,1o,2e,2o); p1 = p3 * (-1)^l2; triangle rule on (l1,l2,l3)
 *   weight rows of class c3: paths ordered by (l1, l2) ascending, channels in order of appearance —
 *   for l <= 1 this is exactly the reference's row order (l1_tensor_prod.py:81-88)
 *   C: real-basis 3j tensors, unit Frobenius norm, basis/sign convention of oracle/cg.py; for l <= 1 they
 *   are the reference's constants (l1_tensor_prod.py:91-94) and xyz dot / cross products.
 * With l <= 1 irreps, lmax_sh = 1 and the same weights/norms, e3_tp_forward == e3_l1tp_forward.
 * ================================================================================================= */
typedef struct e3_tp_plan e3_tp_plan;
/* one column segment of in1 for the fused entry point: rows are base[row_index[b] * ld + c] (row_index NULL = b) */
typedef struct e3_tp_segment {
  const void* base;
  int64_t ld;
  const int32_t* row_index;
  int32_t ncols;
  int32_t reserved;
} e3_tp_segment;
int e3_tp_plan_create(const int32_t* in1_blocks, int n_in1, int lmax_sh,
                      const int32_t* out_blocks, int n_out, e3_tp_plan** plan);
int e3_tp_plan_destroy(e3_tp_plan* plan);
int e3_tp_in1_dim(const e3_tp_plan* plan);
int e3_tp_in2_dim(const e3_tp_plan* plan);
int e3_tp_out_dim(const e3_tp_plan* plan);
/* cls in 0..5; rows = sum of in1 multiplicities over the class's paths ("fan-in"), cols = out multiplicity */
int e3_tp_weight_shape(const e3_tp_plan* plan, int cls, int* rows, int* cols);
int e3_tp_norm_len(const e3_tp_plan* plan, int cls);
int64_t e3_tp_packed_bytes(const e3_tp_plan* plan, int dtype);
int e3_tp_pack_weights(const e3_tp_plan* plan, const void* const weights[6], const void* const norms[6],
                       int dtype, void* packed, void* stream);
/* dtype E3_F32 / E3_F64 (in2 of the same type; ld_in2 == 0 broadcasts row 0) or E3_BF16 (in2 fp32, see below).
 * E3_F32 runs on the matrix cores where the plan has an MFMA instantiation (fp16 (hi, lo)-split operands, fp32
 * accumulation: ~2^-21 per product, see "Operand scales" below); `exact` != 0 forces the generic fp32 FMA kernel.
 * in_scale: device pointer to {s, 1/s} from e3_pow2_scale (NULL = 1: inputs must then lie in about [2^-3, 2^12]). */
int e3_tp_forward(const e3_tp_plan* plan, const void* in1, int64_t ld_in1, const void* in2, int64_t ld_in2,
                  const void* packed, void* out, int64_t ld_out, int64_t B, int dtype, const float* in_scale,
                  int exact, void* stream);
/*
 * Operand scales.  The fp32-storage MFMA kernels split every fp32 operand into two fp16 halves (hi = rne16(v),
 * lo = rne16(v - hi)) and accumulate hi*hi + hi*lo + lo*hi in fp32 on v_mfma_f32_16x16x32_f16.  hi + lo carries 22
 * significant bits while lo is a normal fp16 number, so tensors are multiplied by a power of two that puts their largest
 * magnitude at 2^target (weights: at pack time, 2^13; input features: `in_scale`, 2^10 -- the per-row CG / SH factors
 * add < 2^4).  e3_pow2_scale reduces max |x| over up to 4 fp32 tensors (segs[i].base/ld/ncols x nrows[i]; row_index
 * ignored) and writes out4 = {s, 1/s, scratch, scratch} on the stream; no host synchronisation.  Exact powers of two:
 * scaling itself adds no rounding.  e3_add_pow2_scale: out = h + u (n elements, n % 4 == 0, 16-byte aligned) and the
 * scale of `out` in the same pass (the residual update of a layer yields the next layer's scale for free).
 * The contract, shared by every producer of a scale (these two entries and out_scale4 of e3_tp_forward_fused_epilogue):
 *   - m = max |x| over the FINITE elements only; NaN and +-inf are skipped per element and never hide a finite value
 *     (a tensor with no finite nonzero element gives m = 0).  out4[2] holds the float bits of m.
 *   - e = biased exponent of m.  e == 0 (m zero or denormal) gives s = 1.
 *   - otherwise s = 2^(se - 127) with se = 127 + target_log2 - (e - 127) clamped to [1, 254], i.e. m s lies in
 *     [2^target, 2^(target+1)) unless the clamp bites.  out4[1] = 1/s, exact.
 */
int e3_pow2_scale(const e3_tp_segment* segs, const int64_t* nrows, int nseg, int target_log2, float* out4,
                  void* stream);
int e3_add_pow2_scale(const float* h, const float* u, float* out, int64_t n, int target_log2, float* out4,
                      void* stream);
/*
 * Fused gather + concat (+ gate) form (MFMA kernel, natural-parity irreps 0e/1o/2e only; one plan belongs to the device
 * that was current at its first use -- a call with another current device returns E3_ERR_INVALID_ARG):
 *   in1[b] = [ seg0.base[idx0[b]] | seg1.base[idx1[b]] | ... ]   (the gather and the concat never reach HBM;
 *            segment boundaries must fall on irreps-block boundaries, at most 4 segments)
 *   gate != 0: out irreps must be [32x0e | 32x0e per gated block | 32x1o | 32x2e]; the kernel writes
 *              [silu(s) | sigmoid(g1) v1 | sigmoid(g2) v2] (width 32 + 96 (+160)) instead of the raw TP output.
 * Returns E3_ERR_UNSUPPORTED when the plan / shape has no MFMA instantiation (callers then use
 * e3_gather_concat + e3_tp_forward + e3_gate_blocks).  e3_tp_fused_supported() answers that up front.
 */
int e3_tp_forward_fused(const e3_tp_plan* plan, const e3_tp_segment* segs, int nseg,
                        const void* in2, int64_t ld_in2, const void* packed, void* out, int64_t ld_out,
                        int64_t B, int dtype, int gate, const float* in_scale, void* stream);
/* e3_tp_forward_fused with two epilogue extras, so that a layer's residual update and the next operand scale cost no pass
 * of their own:  out = (gated) product + residual   (residual: [B, width of out], storage dtype, null = none), and
 * out_scale4 (null = none) receives what e3_pow2_scale(out, target_log2) would: {s, 1/s, bits of max |out|, -}. */
int e3_tp_forward_fused_epilogue(const e3_tp_plan* plan, const e3_tp_segment* segs, int nseg, const void* in2,
                                 int64_t ld_in2, const void* packed, void* out, int64_t ld_out, int64_t B, int dtype,
                                 int gate, const float* in_scale, const void* residual, int64_t ld_residual,
                                 float* out_scale4, int target_log2, void* stream);
/* Both products of a SEGNN node update in one launch:  u = gate(plan1([seg0 | seg1 ...] ; in2)),
 * out = plan2(u ; in2) + residual, and out_scale4 (null = none) as in e3_tp_forward_fused_epilogue.  u never reaches HBM.
 * fp32 storage: u's operand scale is a power of two per row (the two-launch path uses one for the whole tensor), so results
 * agree with e3_tp_forward_fused + e3_tp_forward_fused_epilogue to the rounding of the fp16 split, not bit for bit; bf16
 * storage: bit-identical.  E3_ERR_UNSUPPORTED (nothing launched) when the pair has no fused instantiation (plan1 gated with
 * hidden 32 at l_max 2, plan2 = its gated irreps -> hidden irreps, segments without row_index, 16-byte aligned rows):
 * callers then run the two launches. */
int e3_tp_forward_update_pair(const e3_tp_plan* plan1, const e3_tp_plan* plan2, const e3_tp_segment* segs, int nseg,
                              const void* in2, int64_t ld_in2, const void* packed1, const void* packed2,
                              const float* in_scale, const void* residual, int64_t ld_residual, void* out,
                              int64_t ld_out, int64_t B, int dtype, float* out_scale4, int target_log2, void* stream);
/* Gradients of e3_tp_forward (fp32 / fp64; the reference operator relies on torch autograd, l1_tensor_prod.py:240-299).
 * `packed` = the buffer e3_tp_pack_weights wrote for this dtype.  Any of grad_in1 [B, in1_dim] (storage dtype),
 * grad_in2 [B, in2_dim] (ACCUMULATION dtype: fp32 for E3_F32, fp64 for E3_F64; with broadcast in2, ld_in2 == 0, pass
 * ld_gin2 == 0 and a zero-filled [in2_dim] row) and grad_weights[6] (one [rows, cols] array per output class as
 * e3_tp_weight_shape reports, accumulation dtype, ZERO-FILLED by the caller, nullptr to skip a class) may be null.
 * grad_weights (and the broadcast grad_in2) are accumulated with atomics: sums are not bitwise reproducible. */
int e3_tp_backward(const e3_tp_plan* plan, const void* in1, int64_t ld_in1, const void* in2, int64_t ld_in2,
                   const void* packed, const void* grad_out, int64_t ld_gout, void* grad_in1, int64_t ld_gin1,
                   void* grad_in2, int64_t ld_gin2, void* const grad_weights[6], int64_t B, int dtype, void* stream);
/*
 * The same gradients as two thin passes around library GEMMs (the path for large B; fp32 / fp64).  Per output class c3
 * (D3 = 2 l3 + 1, [rows, cols] = e3_tp_weight_shape):
 *   e3_tp_backward_operands   features[c3][b, c, r] = sum_{a,q} C[a][q][c] in1[b,k,a] in2[b,q]   ([B, D3, rows], r = path row + k)
 *                             gout[c3][b, c, w]     = grad_out[b, col(w) + c] * norm[w, c]       ([B, D3, cols])
 *   caller (any GEMM)         grad_W[c3] = features^T gout  over the B * D3 rows;   t[c3] = gout W[c3]^T   ([B, D3, rows])
 *   e3_tp_backward_contract   grad_in1[b,k,a] = sum_paths sum_{q,c} C in2[b,q] t[b,c,r]
 *                             grad_in2[b,q]   = sum_paths sum_{k,a,c} C in1[b,k,a] t[b,c,r]
 * Arrays are dense, accumulation dtype (fp32 / fp64); a null entry skips that class (features / gout) or means the class
 * has no weights (t).  grad_in2 follows e3_tp_backward's convention (accumulation dtype; broadcast in2: ld_in2 == 0,
 * ld_gin2 == 0 and a zero-filled [in2_dim] row, summed with atomics).  Either pointer array of _operands may be null.
 */
/* grad_weights alone, fused (fp32): the features and the normalised output gradient of a row tile are built in LDS and
 * contracted on v_mfma_f32_32x32x2_f32 -- nothing of size [B, D3, rows] reaches HBM.  grad_weights[c]: [rows, cols] fp32,
 * ZERO-FILLED by the caller (sums arrive through atomics), nullptr to skip a class.  E3_ERR_UNSUPPORTED (nothing launched) when a
 * requested class has more than 32 output tiles of 32 x 32 or no row tile fits the LDS: use the operand pass + GEMM then. */
int e3_tp_backward_weights(const e3_tp_plan* plan, const void* in1, int64_t ld_in1, const void* in2, int64_t ld_in2,
                           const void* packed, const void* grad_out, int64_t ld_gout, void* const grad_weights[6],
                           int64_t B, int dtype, void* stream);
int e3_tp_backward_operands(const e3_tp_plan* plan, const void* in1, int64_t ld_in1, const void* in2, int64_t ld_in2,
                            const void* packed, const void* grad_out, int64_t ld_gout, void* const features[6],
                            void* const gout[6], int64_t B, int dtype, void* stream);
int e3_tp_backward_contract(const e3_tp_plan* plan, const void* in1, int64_t ld_in1, const void* in2, int64_t ld_in2,
                            void* const t[6], void* grad_in1, int64_t ld_gin1, void* grad_in2, int64_t ld_gin2,
                            int64_t B, int dtype, void* stream);
int e3_tp_fused_supported(const e3_tp_plan* plan, int gate);
/* kernel family ("e3::tp_fwd_mfma_r16_kernel") that this thread's most recent
 * e3_tp_forward_fused / _scatter / MFMA e3_tp_forward call launched; "" before the first one (diagnostics, bench labels) */
const char* e3_tp_last_fused_kernel(void);
/* e3_tp_forward_fused with the message pass's segment-sum fused into the epilogue: row b of the (gated) product is not
 * stored but ADDED to out_nodes[row_node[b]] (fp32 atomics; row_node ascending, e.g. the dst column of a CSR-by-dst
 * edge list; out_nodes zero-initialised by the caller, ld_out a multiple of 4 elements, 16-byte aligned).  The
 * [B, width] messages never reach HBM.  Summation order is not fixed: results agree with e3_tp_forward_fused +
 * e3_segment_sum to fp32 rounding of the sum, not bit for bit.  out_nodes is FP32 for both storage types (`dtype` is
 * the storage of the inputs; with E3_BF16 the caller rounds the sums once).  gate = 1 only; E3_ERR_UNSUPPORTED when the
 * plan has no two-wave instantiation with this epilogue (callers then run the two kernels). */
int e3_tp_forward_fused_scatter(const e3_tp_plan* plan, const e3_tp_segment* segs, int nseg,
                                const void* in2, int64_t ld_in2, const void* packed, const int32_t* row_node,
                                void* out_nodes, int64_t ld_out, int64_t B, int dtype, int gate,
                                const float* in_scale, void* stream);
/* =================================================================================================
 * Fused SEGNN message function (builder-defined; the north_star's "fused per-edge CDNA4 HIP kernel"):
 *
 *   out[i] = sum_{e: dst[e] = i} gate( TP2( gate( TP1( [h[dst[e]] | h[src[e]] | d_e] ; Y_e ) ) ; Y_e ) )
 *
 * with Y_e, d_e = component spherical harmonics (l <= lmax) and length of pos[src[e]] - pos[dst[e]] (the expressions of
 * e3_edge_geometry / e3_edge_geometry_l2), TP1 / TP2 = e3_tp_* products with in irreps Hx0e+Hx1o(+Hx2e) (TP1: twice that
 * plus 1x0e) and out irreps Hx0e + lmax*H x0e + Hx1o (+Hx2e), gate = [silu(s) | sigmoid(g_l) v_l].  One launch (plus a
 * per-node pre-mix launch) per layer: neither Y [E, 9], d [E] nor any [E, width] message tensor exists in HBM.
 * hidden in {16, 32, 64}.  dtype E3_F32: fp32 storage, fp16 (hi, lo)-split MFMA products (see "Operand scales"; `in_scale` =
 * scale of h, NULL = 1; the gated messages between the two products are scaled per edge row inside the kernel).
 * dtype E3_BF16 (hidden 32 / 64; e3_msg_supports): h, weights and norms bf16, positions / harmonics / accumulators / the
 * pre-mix table / `out` fp32, one bf16 MFMA per product, the messages between the two products rounded to bf16.
 * Edges must be sorted by dst (CSR order, as e3_rg_fill emits them): runs of equal dst are summed on chip and leave as
 * one fp32 atomic add per node and wave -- sums agree with e3_segment_sum to fp32 rounding, not bit for bit.
 *   weights: w1[l3] / w2[l3] = the class matrices of TP1 / TP2 for output degree l3 (0e, 1o, 2e), row order and shapes
 *            as e3_tp_weight_shape reports for those irreps (e3_msg_weight_shape returns the same numbers);
 *            n1 / n2 = their norm buffers (length M, 3 M, 5 M) or NULL for 1.
 *   premix : N * e3_msg_premix_floats_per_node() floats written by e3_msg_premix; call e3_msg_premix(h) before
 *            e3_msg_forward on the same h and in_scale.  Three regions, in this order (e3_msg_premix_regions reports the
 *            offsets; the entries take no size: N * e3_msg_premix_floats_per_node() floats are the caller's contract):
 *              [N x UD floats]  the table W_dst h per node: the dst half of TP1 does not depend on the edge, so it is
 *                               contracted once per NODE and enters the edge kernel as the MFMA accumulator's initial value
 *              [N x S floats]   the pre-split rows, S = 32 (l_max + 1)^2 for plans whose fp32 edge kernel is the
 *                               weights-stationary one (hidden = 32, l_max = 2), else S = 0: h[n] * in_scale as the fp16
 *                               (hi, lo) B fragments that kernel gathers per edge instead of converting h[src].  Per node
 *                               (l_max + 1)^2 fragments (component l^2 + a) of 128 bytes: 4 x 16 bytes of hi halves (k
 *                               group g = 0 .. 3: 8 fp16, channels 4 g .. 4 g + 3 then 16 + 4 g .. 16 + 4 g + 3), then the
 *                               4 x 16 bytes of lo halves; hi = rne16(x), lo = rne16(x - hi).  Written for fp32 storage only
 *                               (bf16 storage leaves the region unused).
 *              [N floats]       max |h[n] * in_scale| per node, from which the edge kernel bounds a row's messages
 *            UD * 4 and S * 4 are multiples of 128, so every region of a 128-byte aligned buffer starts on a cache line
 *            (recommended; 16-byte alignment is required).
 *            Rows of h that change after e3_msg_premix and are only gathered as src rows afterwards (ghost rows after a halo
 *            exchange): e3_msg_refresh_rows(rows[n_rows], int64 node ids) rewrites their pre-split row and row maximum
 *            (maximum over the finite values); ids outside [0, N) are skipped.
 *   out    : [N, ld_out] fp32, columns [H | 3 H | 5 H]; zero-filled by the call unless accumulate != 0
 *   accumulate != 0: a second edge list for the SAME h rows of the dst nodes (e.g. the halo's boundary edges after the
 *            interior ones): out keeps its contents (premix is reused: it depends on dst rows only)
 *   tiles_per_block: work granularity (0 = default).  hidden = 32, l_max = 2, fp32: the weights-stationary kernel
 *            (e3_msg_ws.hip: one workgroup of 8 waves per CU walks chunks of 16 * tiles_per_block edges, default 256 edges,
 *            dealt round-robin to the workgroups of an XCD; tiles inside a chunk are cut at dst-run boundaries: <= 16 edges,
 *            <= 2 runs).  Other shapes, or tiles_per_block < 0: the one-wave-per-tile kernel (e3_msg_fused_kernel.h), where
 *            |tiles_per_block| = consecutive 16-edge tiles a wave processes before it jumps to its workgroup's next chunk (0 = 4)
 *   E      : edges of this call, dst-sorted (src / dst int32); E <= 2^31 - 17 (E3_ERR_INVALID_ARG beyond: the edge ids are
 *            int32 and the kernel's tile arithmetic is 32-bit)
 *   The launch fills the device once: one 512-thread workgroup per CU (weights-stationary kernel), or CUs x the workgroups
 *   per CU that hipOccupancyMaxActiveBlocksPerMultiprocessor reports for the kernel's registers and LDS image (queried at
 *   the plan's first use).
 * One plan belongs to the device current at its first use.
 * ================================================================================================= */
typedef struct e3_msg_plan e3_msg_plan;
int e3_msg_plan_create(int lmax, int hidden, e3_msg_plan** plan);
int e3_msg_plan_destroy(e3_msg_plan* plan);
int64_t e3_msg_packed_bytes(const e3_msg_plan* plan);
int64_t e3_msg_premix_floats_per_node(const e3_msg_plan* plan);
int e3_msg_weight_shape(const e3_msg_plan* plan, int tp /* 1 | 2 */, int l3, int* rows, int* cols);
int e3_msg_supports(const e3_msg_plan* plan, int dtype);
int e3_msg_pack_weights(e3_msg_plan* plan, const void* const w1[3], const void* const n1[3],
                        const void* const w2[3], const void* const n2[3], int dtype, void* packed, void* stream);
int e3_msg_premix(e3_msg_plan* plan, const void* h, int64_t ld_h, int64_t N, const void* packed,
                  const float* in_scale, float* premix, int dtype, void* stream);
int e3_msg_premix_regions(const e3_msg_plan* plan, int64_t N, int64_t* split_offset, int64_t* split_floats_per_node,
                          int64_t* row_max_offset); /* offsets in floats; any output may be NULL */
int e3_msg_refresh_rows(e3_msg_plan* plan, const void* h, int64_t ld_h, int64_t N, const int64_t* rows, int64_t n_rows,
                        const float* in_scale, float* premix, int dtype, void* stream);
int e3_msg_forward(e3_msg_plan* plan, const void* h, int64_t ld_h, int64_t N, const float* pos4,
                   const int32_t* src, const int32_t* dst, int64_t E, const void* packed, const float* in_scale,
                   const float* premix, float* out, int64_t ld_out, int dtype, int accumulate, int tiles_per_block,
                   void* stream);
/* e3_msg_forward with Y_e, d_e of the minimum-image edge vector (box[3] as in e3_edge_geometry_pbc) */
int e3_msg_forward_pbc(e3_msg_plan* plan, const void* h, int64_t ld_h, int64_t N, const float* pos4,
                       const int32_t* src, const int32_t* dst, int64_t E, const void* packed, const float* in_scale,
                       const float* premix, float* out, int64_t ld_out, int dtype, int accumulate, int tiles_per_block,
                       const float box[3], void* stream);
/* e3_msg_forward with Y_e, d_e of the minimum image in a general cell (cell[9] as in e3_rg_sort_count_cell) */
int e3_msg_forward_cell(e3_msg_plan* plan, const void* h, int64_t ld_h, int64_t N, const float* pos4,
                        const int32_t* src, const int32_t* dst, int64_t E, const void* packed, const float* in_scale,
                        const float* premix, float* out, int64_t ld_out, int dtype, int accumulate, int tiles_per_block,
                        const float cell[9], void* stream);
/*
 * Owned sums: e3_msg_forward for a launch that does not accumulate, with every row of `out` written exactly once -- no
 * zero-fill, no atomics -- and the operand scale of `out` from the same launches.  The edges are dst-sorted and a chunk of
 * the weights-stationary kernel is a contiguous edge range, so a node whose run lies strictly inside a chunk is complete when
 * the kernel flushes it: the kernel stores such rows itself.  The first and the last node of every chunk go through a
 * boundary buffer in `workspace` and are summed in edge order by a small kernel; a second one zeroes the rows of nodes
 * without an incoming edge (one pass over dst).  Sums are reproducible from run to run, and bit-identical to
 * e3_msg_forward's for every node with at most two partial sums.
 *   workspace : e3_msg_owned_workspace_bytes(plan, E, dtype, tiles_per_block) bytes, 16-byte aligned, scratch of the call
 *               (-1: the shape / tiles_per_block < 0 does not run the weights-stationary kernel; the forward entries then
 *               return E3_ERR_UNSUPPORTED with nothing launched: use e3_msg_forward + e3_pow2_scale)
 *   out_scale4: receives what e3_pow2_scale(out [N, D], target_log2) would (the contract above e3_pow2_scale):
 *               {s, 1/s, bits of max |out| over the finite elements, -}
 * Everything else as e3_msg_forward / _pbc / _cell with accumulate = 0.
 */
int64_t e3_msg_owned_workspace_bytes(const e3_msg_plan* plan, int64_t E, int dtype, int tiles_per_block);
int e3_msg_forward_owned(e3_msg_plan* plan, const void* h, int64_t ld_h, int64_t N, const float* pos4,
                         const int32_t* src, const int32_t* dst, int64_t E, const void* packed, const float* in_scale,
                         const float* premix, float* out, int64_t ld_out, int dtype, int tiles_per_block,
                         void* workspace, int64_t workspace_bytes, float* out_scale4, int target_log2, void* stream);
int e3_msg_forward_owned_pbc(e3_msg_plan* plan, const void* h, int64_t ld_h, int64_t N, const float* pos4,
                             const int32_t* src, const int32_t* dst, int64_t E, const void* packed,
                             const float* in_scale, const float* premix, float* out, int64_t ld_out, int dtype,
                             int tiles_per_block, void* workspace, int64_t workspace_bytes, float* out_scale4,
                             int target_log2, const float box[3], void* stream);
int e3_msg_forward_owned_cell(e3_msg_plan* plan, const void* h, int64_t ld_h, int64_t N, const float* pos4,
                              const int32_t* src, const int32_t* dst, int64_t E, const void* packed,
                              const float* in_scale, const float* premix, float* out, int64_t ld_out, int dtype,
                              int tiles_per_block, void* workspace, int64_t workspace_bytes, float* out_scale4,
                              int target_log2, const float cell[9], void* stream);
/*
 * bf16 storage (dtype E3_BF16, BASELINE config 3): segments / in1 / out / weights / norms are bf16, in2 (the
 * spherical harmonics) stays fp32, products run once on v_mfma_f32_16x16x32_bf16 with fp32 accumulation and one
 * rounding of the result.  Only the MFMA path exists for bf16 (E3_ERR_UNSUPPORTED otherwise).
 */
int e3_segment_sum_bf16(const void* msg, int64_t ld_msg, const int32_t* rowptr, int64_t N, int D,
                        void* agg, int64_t ld_agg, void* stream);
/* SH / geometry for lmax 2: edge_y [E,9], node_a [N,9] (same definitions as e3_edge_geometry, Y2 = sqrt5 b(r^)) */
int e3_edge_geometry_l2(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N,
                        float* edge_y, float* edge_d, float* node_a, void* stream);
/* periodic box: as e3_edge_geometry_pbc */
int e3_edge_geometry_l2_pbc(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, const float box[3],
                            float* edge_y, float* edge_d, float* node_a, void* stream);
/* general cell: as e3_edge_geometry_cell */
int e3_edge_geometry_l2_cell(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, const float cell[9],
                             float* edge_y, float* edge_d, float* node_a, void* stream);
/* general gate: in = [ns scalars | g gate scalars | gated blocks], block i = mul_i x (2 l_i + 1) with one gate per
 * channel, gates consumed in block order; out = [silu(s) | sigmoid(gate) * block].  ls/muls: host int arrays. */
int e3_gate_blocks(const float* in, int64_t ld_in, float* out, int64_t ld_out, int64_t B, int ns,
                   int nblocks, const int32_t* ls, const int32_t* muls, void* stream);

/* =================================================================================================
 * Backward of the edge / node stages (fp32): with e3_l1tp_backward / e3_tp_backward they make a whole SEGNN layer
 * differentiable, i.e. parameter gradients and the force head -dE/dpos (BASELINE.json configs[3]).  The reference's
 * contract for its own operator is torch autograd (l1_tensor_prod.py:234-299); these are the same for the stages it lacks.
 *   e3_edge_geometry_backward : g_pos [N,3] (zero-filled by the call) from g_edge_y [E,(lmax+1)^2], g_edge_d [E],
 *                               g_node_a [N,(lmax+1)^2] (any may be NULL); atomics on g_pos.
 *   e3_gather_concat_backward : g_out [E, 2D+n_extra] -> g_h [N,D] (zero-filled by the call; dst rows summed per CSR row,
 *                               src rows by atomics), g_extra [E,n_extra] (may be NULL).
 *   e3_gate_blocks_backward   : in = the forward's input [B, ns+ngates+wide], g_out [B, ns+wide] -> g_in (same layout
 *                               as in); e3_gate is the one-block case {l = 1, mul = nv}.
 *   e3_segment_sum_backward   : g_msg[e] = g_agg[dst(e)].
 * ================================================================================================= */
int e3_edge_geometry_backward(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                              const float* g_edge_y, const float* g_edge_d, const float* g_node_a, float* g_pos,
                              void* stream);
/* periodic box: as e3_edge_geometry_pbc */
int e3_edge_geometry_backward_pbc(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                  const float box[3], const float* g_edge_y, const float* g_edge_d,
                                  const float* g_node_a, float* g_pos, void* stream);
/* general cell: as e3_edge_geometry_cell */
int e3_edge_geometry_backward_cell(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                   const float cell[9], const float* g_edge_y, const float* g_edge_d,
                                   const float* g_node_a, float* g_pos, void* stream);
int e3_gather_concat_backward(const float* g_out, int64_t ld_gout, int D, const int32_t* rowptr, const int32_t* src,
                              int64_t N, int n_extra, float* g_h, int64_t ld_gh, float* g_extra, void* stream);

/* =================================================================================================
 * Strain, virial and stress (first order).  Structure s of an edge = structure of its dst row (structure[dst], NULL = every
 * row is structure 0); each structure has a 3x3 strain eps_s (strain [S,9] fp32 on the device, row-major eps[3 a + b]).
 * With r_e the edge vector of the undeformed graph (open box: x_src - x_dst; box != NULL: its minimum image exactly as in
 * e3_edge_geometry_pbc), the strained vector is
 *   r'_e = r_e + eps_s r_e      (fp32, per component  r'_a = r_a + (eps[3a] r_0 + eps[3a+1] r_1 + eps[3a+2] r_2))
 * and Y_e, d_e and A_i are those of r'_e; the edge set is the one of the undeformed graph.  The derivative at eps = 0 is
 * exact; a finite eps is a first-order tool (finite differences).  At eps = 0 the outputs equal the unstrained entries'.
 *   dE/deps_s[a,b] = sum over the edges e of s of (dE/dr'_e)_a (r_e)_b
 *   virial W_s = -dE/deps_s at eps = 0 (not symmetrised: its symmetry is a check);
 *   stress sigma = (1/V) dE/deps at eps = 0, V = L_x L_y L_z, all three axes periodic (ASE / NequIP / MACE: sigma = -W/V).
 * Rows with no edges and edges with d = 0 contribute nothing.  A row whose structure id is outside [0, S) reads no strain
 * and writes no strain gradient: it is computed unstrained.  Units: those of E and pos.
 * lmax 1 or 2 (edge_y [E,(lmax+1)^2], node_a [N,(lmax+1)^2]); box: host float[3] as in e3_edge_geometry_pbc, or NULL for an
 * open box.  E3_ERR_INVALID_ARG before any launch for lmax outside {1, 2}, strain NULL, S < 1 or an invalid box.
 * ================================================================================================= */
int e3_edge_geometry_strained(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                              const float* box, const float* strain, const int32_t* structure, int S, float* edge_y,
                              float* edge_d, float* node_a, void* stream);
/* bytes of the backward's workspace for N rows (needed when S = 1; 9 floats per workgroup, at most 147 456 B) */
int64_t e3_edge_geometry_backward_strained_workspace_bytes(int64_t N);
/* Backward of e3_edge_geometry_strained in one pass: g_pos [N,3] (zero-filled by the call; (I + eps_s)^T of the gradient at
 * r', atomics as e3_edge_geometry_backward) and g_strain [S,9] = dE/deps_s (zero-filled by the call).
 * S = 1: per-wave register sums and per-workgroup LDS sums written to `workspace`, then a second pass adds them in a fixed
 * order: g_strain is bitwise reproducible from run to run.  S > 1 (e.g. batched molecules, whose rows are not contiguous
 * in graph order): one wave reduction per row and one 9-lane atomic add into g_strain[s]: the sums depend on the order of
 * arrival.  E3_ERR_INVALID_ARG also for g_strain NULL or, when S = 1 and N > 0, a workspace smaller than
 * e3_edge_geometry_backward_strained_workspace_bytes(N). */
int e3_edge_geometry_backward_strained(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                       const float* box, const float* strain, const int32_t* structure, int S,
                                       const float* g_edge_y, const float* g_edge_d, const float* g_node_a, float* g_pos,
                                       float* g_strain, void* workspace, int64_t workspace_bytes, void* stream);
/* The strained pair in a general cell (cell[9] as in e3_rg_sort_count_cell, required): r_e = the cell's minimum image,
 * stress = (1/V) dE/deps with V = |det cell|.  Same outputs, workspace (e3_edge_geometry_backward_strained_workspace_bytes)
 * and reproducibility contract (S = 1 fixed order, S > 1 atomics) as the two entries above. */
int e3_edge_geometry_strained_cell(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                   const float cell[9], const float* strain, const int32_t* structure, int S,
                                   float* edge_y, float* edge_d, float* node_a, void* stream);
int e3_edge_geometry_backward_strained_cell(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N,
                                            int lmax, const float cell[9], const float* strain, const int32_t* structure,
                                            int S, const float* g_edge_y, const float* g_edge_d, const float* g_node_a,
                                            float* g_pos, float* g_strain, void* workspace, int64_t workspace_bytes,
                                            void* stream);
int e3_gate_blocks_backward(const float* in, int64_t ld_in, const float* g_out, int64_t ld_gout, float* g_in,
                            int64_t ld_gin, int64_t B, int ns, int nblocks, const int32_t* ls, const int32_t* muls,
                            void* stream);
int e3_segment_sum_backward(const float* g_agg, int64_t ld_gagg, const int32_t* rowptr, int64_t N, int D, float* g_msg,
                            int64_t ld_gmsg, void* stream);

/* =================================================================================================
 * Smooth cutoff envelope (fp32): the weight of an edge in the aggregation of an energy model, so that the energy is a
 * twice continuously differentiable function of the positions when a pair crosses the cutoff r_c.  Polynomial envelope with
 * an integer 2 <= p <= 16 (6 is the usual choice):
 *   x        = min(fl(d * fl(1 / r_c)), 1)
 *   u_p(x)   = (1 - x)^3 * sum_{k=0}^{p-1} C(k+2, 2) x^k          (the sum by Horner from k = p-1 down)
 *   du/dd    = -(p (p+1) (p+2) / 2) * x^(p-1) * (1 - x)^2 / r_c
 * This is the DimeNet polynomial 1 - (p+1)(p+2)/2 x^p + p(p+2) x^(p+1) - p(p+1)/2 x^(p+2) in a form without cancellation
 * (the expanded form loses most of its digits near x = 1 and is not evaluated).  u(0) = 1; u = u' = u'' = 0 at x = 1;
 * du/dd = 0 at d = 0.  Every d >= r_c gives w = 0 and g_d = 0 EXACTLY (a compare on d, not the rounding of x), so a graph
 * built with a skin (r_c + skin) gives the energy of the graph built at r_c.  A NaN d gives a NaN w.
 *   e3_cutoff_envelope          : w[e] = u_p(x(edge_d[e]))
 *   e3_cutoff_envelope_backward : g_d[e] = g_w[e] * du/dd(edge_d[e])
 * E3_ERR_INVALID_ARG before any launch for p outside [2, 16], r_c not finite or <= 0 (or 1 / r_c not finite) and E < 0;
 * E = 0 returns E3_OK.
 *
 * Weighted segment sum: the aggregation with the envelope, and its backward.  Rows = CSR rows of the graph (dst nodes),
 * D columns, row strides in elements.
 *   e3_segment_sum_weighted          : agg[i] = sum over CSR row i of w[e] * msg[e], edges in row order, one
 *                                      fmaf(w, m, acc) per element and edge from acc = 0.  Bit-equal from run to run; with
 *                                      every w = 1 bit-equal to e3_segment_sum.  Rows without edges are zero.
 *   e3_segment_sum_weighted_backward : g_msg[e] = w[e] * g_agg[dst(e)] (one rounding per element);
 *                                      g_w[e] = <msg[e], g_agg[dst(e)]> over the D columns (g_w may be NULL: msg is then
 *                                      not read and may be NULL): per lane over its columns in column order, then a
 *                                      shuffle butterfly over the 64 lanes -- a fixed order, no atomics: bit-equal from
 *                                      run to run.
 * 16-byte loads and stores per lane when D, every stride and every base pointer is a multiple of 4 elements / 16 bytes,
 * 4-byte ones otherwise (same sums, same order).  E3_ERR_INVALID_ARG before any launch for N < 0, D <= 0 or a stride
 * below D; N = 0 returns E3_OK.
 * ================================================================================================= */
int e3_cutoff_envelope(const float* edge_d, int64_t E, float r_c, int p, float* w, void* stream);
int e3_cutoff_envelope_backward(const float* edge_d, const float* g_w, int64_t E, float r_c, int p, float* g_d,
                                void* stream);
int e3_segment_sum_weighted(const float* msg, int64_t ld_msg, const float* w, const int32_t* rowptr, int64_t N, int D,
                            float* agg, int64_t ld_agg, void* stream);
int e3_segment_sum_weighted_backward(const float* g_agg, int64_t ld_gagg, const float* msg, int64_t ld_msg, const float* w,
                                     const int32_t* rowptr, int64_t N, int D, float* g_msg, int64_t ld_gmsg, float* g_w,
                                     void* stream);

/* =================================================================================================
 * Second derivatives (fp32): what the backward of the stage backwards above needs besides those entries themselves, so that
 * a loss on the forces F = -dE/dpos has parameter gradients.  The tensor products, gather/concat and the segment sums are
 * multilinear: their double backward is the existing entries with one argument replaced by a cotangent.  New arithmetic:
 *
 *   e3_edge_geometry_jvp : e3_edge_geometry_backward is linear in (g_edge_y, g_edge_d, g_node_a), so the cotangents of those
 *       three for a cotangent v [N,3] of g_pos are the tangent of the forward along the displacement field v.  Per edge
 *       t_e = v[src] - v[dst] (r_e, u_e, d_e as in the forward: the minimum image in a box or cell, whose shift is piecewise
 *       constant):  d_edge_d[e] = u_e . t_e;  d_edge_y[e,k] = (dY_k/dr) t_e with du/dr = (I - u u^T) / d and the b(u) of
 *       e3_edge_geometry_l2, d_edge_y[e,0] = 0;  d_node_a[i,k] = (1/deg_i) sum over CSR row i of d_edge_y[e,k],
 *       d_node_a[i,0] = 0.  Edges with d = 0 and rows without edges give zeros.  Each of the three outputs may be NULL.  One
 *       wave per row; d_node_a is one fixed-order wave reduction per row (no atomics): bit-equal from run to run.  The
 *       derivative of g_pos w.r.t. pos itself is e3_edge_geometry_hvp below.
 *       E3_ERR_INVALID_ARG for lmax outside {1, 2}, N < 0, an invalid box / cell, or (N > 0) a NULL pos4 / rowptr / src / v.
 *
 *   e3_edge_geometry_hvp : the other half of the backward of e3_edge_geometry_backward, its vector-Jacobian product in the
 *       positions: h_pos = d<v, g_pos(pos; g_edge_y, g_edge_d, g_node_a)>/dpos for a cotangent v [N,3] of g_pos -- with the
 *       cotangents above, everything a Hessian-vector product of the energy needs.  Per edge (r_e the minimum image, whose
 *       shift is piecewise constant; d = |r|, u = r / d; g = g_edge_y[e] + g_node_a[dst] / deg on the components >= 1) the
 *       first-order edge gradient is grad phi_e, phi_e(r) = <g, Y(r)> + g_edge_d[e] |r|, and
 *         h_e = (Hess phi_e) t_e,  t_e = v[src] - v[dst];   h_pos[src] += h_e,  h_pos[dst] -= h_e.
 *       On the unit sphere <g, Y> = a1 . u + u^T Q u / 2 with a1 = sqrt3 (g1, g2, g3) and (l_max = 2; Q = 0 at l_max = 1)
 *         Q = sqrt5 [[-g6 + sqrt3 g8, sqrt3 g4, sqrt3 g7], [sqrt3 g4, -g6 - sqrt3 g8, sqrt3 g5], [sqrt3 g7, sqrt3 g5, 2 g6]],
 *       so with psi = a1 + Q u (the g_u of e3_edge_geometry_backward), P = I - u u^T, du = P t / d and dd = u . t:
 *         h_e = [ -(du (u . psi) + u (du . psi)) + P Q du ] / d  -  P psi dd / d^2  +  g_edge_d[e] du.
 *       Each of g_edge_y, g_edge_d, g_node_a may be NULL (zeros), as in e3_edge_geometry_backward.  Edges with d = 0 and rows
 *       without edges contribute nothing.  h_pos [N,3] is zero-filled by the call.  One wave per dst row, lanes over its
 *       edges: fp32 atomics into h_pos[src], a wave reduction and one atomic per component for the dst row -- like g_pos, the
 *       result is NOT bit-reproducible on a general cloud (order of arrival).  The strained form is
 *       e3_edge_geometry_hvp_strained below.
 *       E3_ERR_INVALID_ARG before any launch for lmax outside {1, 2}, N < 0, a NULL v or h_pos, an invalid box / cell, or
 *       (N > 0) a NULL rowptr, or a NULL pos4 with a src; N = 0, or a NULL src (a graph without edges): zero-fill only.
 *
 *   e3_gate_blocks_backward2 : in, g_out as e3_gate_blocks_backward, c = the cotangent of its g_in (layout of in).  With
 *       s = sigmoid, one launch writes cot_g_out (layout of g_out) and cot_in (layout of in), either may be NULL:
 *         scalars  cot_g_out = c silu'(x),  cot_in = c g_out silu''(x),  silu'' = s' (2 + x (1 - 2 s)),  s' = s (1 - s)
 *         gated    cot_g_out[v_m] = s(g) c[v_m] + s'(g) c[g] v_m,       cot_in[v_m] = s'(g) c[g] g_out[v_m]
 *         gate     cot_in[g] = s'(g) sum_m c[v_m] g_out[v_m] + s''(g) c[g] sum_m v_m g_out[v_m],  s'' = s' (1 - 2 s)
 *
 *   e3_cutoff_envelope_backward2 : c = the cotangent of e3_cutoff_envelope_backward's g_d.  cot_g_w[e] = c du/dd,
 *       cot_d[e] = c g_w d2u/dd2,  d2u/dd2 = -(p (p+1) (p+2) / 2) / r_c^2 * x^(p-2) (1 - x) ((p-1) (1 - x) - 2 x)  (x^0 = 1);
 *       both EXACTLY 0 for d >= r_c.  Either output may be NULL (g_w is not read when cot_d is NULL).
 * ================================================================================================= */
int e3_edge_geometry_jvp(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax, const float* v,
                         float* d_edge_y, float* d_edge_d, float* d_node_a, void* stream);
/* periodic box: as e3_edge_geometry_pbc */
int e3_edge_geometry_jvp_pbc(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                             const float box[3], const float* v, float* d_edge_y, float* d_edge_d, float* d_node_a,
                             void* stream);
/* general cell: as e3_edge_geometry_cell */
int e3_edge_geometry_jvp_cell(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                              const float cell[9], const float* v, float* d_edge_y, float* d_edge_d, float* d_node_a,
                              void* stream);
int e3_edge_geometry_hvp(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                         const float* g_edge_y, const float* g_edge_d, const float* g_node_a, const float* v, float* h_pos,
                         void* stream);
/* periodic box: as e3_edge_geometry_pbc */
int e3_edge_geometry_hvp_pbc(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                             const float box[3], const float* g_edge_y, const float* g_edge_d, const float* g_node_a,
                             const float* v, float* h_pos, void* stream);
/* general cell: as e3_edge_geometry_cell */
int e3_edge_geometry_hvp_cell(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                              const float cell[9], const float* g_edge_y, const float* g_edge_d, const float* g_node_a,
                              const float* v, float* h_pos, void* stream);
/* The two entries above for the strained geometry: the backward of e3_edge_geometry_backward_strained (conventions of
 * e3_edge_geometry_strained: r the unstrained edge vector, s the structure of the dst row, M = I + eps_s, r' = M r; box NULL
 * = open box).  Cotangents v [N,3] of g_pos and xi [S,9] of g_strain (row-major as strain); either may be NULL (zeros), not
 * both.  With t_e = v[src] - v[dst] the tangent of r' is
 *   t'_e = M t_e + xi_s r_e.
 *   e3_edge_geometry_jvp_strained : the cotangents of (g_edge_y, g_edge_d, g_node_a) are the outputs of e3_edge_geometry_jvp
 *       with u, d taken at r' and t := t'.  Same NULL outputs, zeros and reproducibility as that entry.
 *   e3_edge_geometry_hvp_strained : with g' = grad phi_e(r') (the first-order edge gradient) and w_e = (Hess phi_e)(r') t'_e
 *       (the h_e formula of e3_edge_geometry_hvp at r'),
 *         h_e = M^T w_e + xi_s^T g'_e;   h_pos[src] += h_e,  h_pos[dst] -= h_e;
 *         h_strain[s][3 a + b] += (w_e)_a (r_e)_b + (g'_e)_a (t_e)_b.
 *       h_pos [N,3] and h_strain [S,9] are zero-filled by the call; either may be NULL (not formed), not both.  h_strain is
 *       reduced as g_strain is: S = 1 through `workspace` (e3_edge_geometry_backward_strained_workspace_bytes(N): the grid is
 *       that of the strained backward) in a fixed order -- bit-equal from run to run; S > 1 one wave reduction per row and one
 *       9-lane atomic (order of arrival).  h_pos: atomics, as e3_edge_geometry_hvp.
 * A row whose structure id is outside [0, S) is computed unstrained (M = I, no xi r term) and adds nothing to h_strain; edges
 * with d' = 0 and rows without edges contribute nothing and give zeros in the tangent.  At eps = 0 and xi = NULL the outputs
 * equal the unstrained entries' (h_strain beside them: the derivative of <v, g_pos> in the strain).
 * E3_ERR_INVALID_ARG before any launch for what the unstrained entries refuse (apart from a NULL v), strain NULL, S < 1, v and
 * xi both NULL, (hvp) h_pos and h_strain both NULL, or, when S = 1, N > 0 and h_strain is given, a workspace that is NULL or
 * too small.  N = 0, or (hvp) a NULL src: zero-fill only. */
int e3_edge_geometry_jvp_strained(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                  const float* box, const float* strain, const int32_t* structure, int S, const float* v,
                                  const float* xi, float* d_edge_y, float* d_edge_d, float* d_node_a, void* stream);
/* general cell: as e3_edge_geometry_strained_cell */
int e3_edge_geometry_jvp_strained_cell(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                       const float cell[9], const float* strain, const int32_t* structure, int S,
                                       const float* v, const float* xi, float* d_edge_y, float* d_edge_d, float* d_node_a,
                                       void* stream);
int e3_edge_geometry_hvp_strained(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                  const float* box, const float* strain, const int32_t* structure, int S,
                                  const float* g_edge_y, const float* g_edge_d, const float* g_node_a, const float* v,
                                  const float* xi, float* h_pos, float* h_strain, void* workspace, int64_t workspace_bytes,
                                  void* stream);
/* general cell: as e3_edge_geometry_strained_cell */
int e3_edge_geometry_hvp_strained_cell(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                       const float cell[9], const float* strain, const int32_t* structure, int S,
                                       const float* g_edge_y, const float* g_edge_d, const float* g_node_a, const float* v,
                                       const float* xi, float* h_pos, float* h_strain, void* workspace,
                                       int64_t workspace_bytes, void* stream);
int e3_gate_blocks_backward2(const float* in, int64_t ld_in, const float* g_out, int64_t ld_gout, const float* c,
                             int64_t ld_c, float* cot_g_out, int64_t ld_cgout, float* cot_in, int64_t ld_cin, int64_t B,
                             int ns, int nblocks, const int32_t* ls, const int32_t* muls, void* stream);
int e3_cutoff_envelope_backward2(const float* edge_d, const float* g_w, const float* c, int64_t E, float r_c, int p,
                                 float* cot_g_w, float* cot_d, void* stream);

/* =================================================================================================
 * Verlet neighbour list (neighbor_list.NeighborList): a graph of e3_rg_* built once at the radius r + skin is cut down, on
 * the device, to the pairs within r at the current positions -- an ordinary CSR graph at radius r in the stored graph's node
 * order -- and the largest displacement since the build comes back with it.  One entry per periodicity mode (box[3] as in
 * e3_edge_geometry_pbc, cell[9] as in e3_rg_sort_count_cell).
 *   inputs  : pos [N,3] fp32, the CURRENT positions in the caller's order (periodic coordinates may be unwrapped);
 *             perm [N], ref_pos4 [N,4], rowptr [N+1], src [E]: the stored graph (ref_pos4 = its sorted_pos4).
 *   outputs : pos4_out [N,4] = (pos[perm[i]], 0);  rowptr_out [N+1], src_out / dst_out (room for E each: the pruned count
 *             can only be smaller, so no host read sizes them);  stats [2] uint32 (device):
 *             stats[0] = the fp32 bits, sign cleared, of max_i d2_i;  stats[1] = rowptr_out[N], the pruned edge count.
 * Every fp32 operation is rounded on its own (no FMA contraction):
 *   displacement : D_i = the minimum image of fl(pos[perm[i]] - ref_i) in the rint form of `rel` above (per periodic axis
 *             fl(d - fl(L rintf(fl(d invL)))); in a cell shift(d, rintf(frac(d))); the identity on an open axis or box), so
 *             re-wrapping the positions between two calls moves nothing.  d2_i = fl(fl(fl(Dx Dx) + fl(Dy Dy)) + fl(Dz Dz)).
 *             Non-negative floats order as their unsigned bits and a NaN pattern orders above +inf: the maximum is taken on
 *             the bits (per wave, per block, then one atomic max per block), and a non-finite position reads as larger
 *             than every threshold.  stats is zeroed on the stream inside the entry.
 *   edge    : edge e = (src_e -> row i) of the stored graph is kept iff d2 <= fl(r r), with rel = the edge vector of the
 *             geometry kernels at pos4_out[src_e], pos4_out[i] and d2 = fl(fl(fl(rx rx) + fl(ry ry)) + fl(rz rz)): the
 *             builder's sum order.  In an open box at unchanged positions this is the builder's test as written (rel is
 *             its dx negated, which is exact) and bit for bit its restatement; the builder's file is compiled with FMA
 *             contraction and this one without, so the two compiled d2 may differ by an ulp for a pair that close to the
 *             cutoff -- which the 2^-10 below covers.
 *   order   : rows in the stored order; the kept src of a row keep their order (ascending); dst_out[e] = the row of e.
 * The caller decides from stats[0] whether the stored graph still covers the cutoff.  With skin the margin the graph was
 * built with and h = 0.5 skin (1 - 2^-10): while every d2_i < fl(h h), every pair within r now was within r + skin at the
 * build, hence is in the stored graph, and the pruned graph is the radius graph at r.  The 2^-10 pays for the roundings of
 * D_i, of rel and of the builder's dx -- together below 64 * 2^-24 X for coordinates (and box / cell extents) of magnitude
 * at most X -- so the argument holds for X <= 2^8 skin.
 * E3_ERR_INVALID_ARG before any launch for a NULL pointer (the node arrays may be NULL when N = 0, the edge arrays when
 * E = 0), N + 1 or E outside int32, r not finite or <= 0, and a box / cell that e3_edge_geometry_pbc / _cell reject.
 * N = 0 launches nothing and writes stats = {0, 0} and rowptr_out[0] = 0.  workspace = e3_nl_workspace_bytes(N) bytes
 * (-1 for N outside int32).
 * ================================================================================================= */
int64_t e3_nl_workspace_bytes(int64_t N);
int e3_nl_update(const float* pos, const int32_t* perm, const float* ref_pos4, const int32_t* rowptr, const int32_t* src,
                 int64_t N, int64_t E, float r, float* pos4_out, int32_t* rowptr_out, int32_t* src_out, int32_t* dst_out,
                 uint32_t* stats, void* workspace, void* stream);
int e3_nl_update_pbc(const float* pos, const int32_t* perm, const float* ref_pos4, const int32_t* rowptr, const int32_t* src,
                     int64_t N, int64_t E, float r, const float box[3], float* pos4_out, int32_t* rowptr_out,
                     int32_t* src_out, int32_t* dst_out, uint32_t* stats, void* workspace, void* stream);
int e3_nl_update_cell(const float* pos, const int32_t* perm, const float* ref_pos4, const int32_t* rowptr, const int32_t* src,
                      int64_t N, int64_t E, float r, const float cell[9], float* pos4_out, int32_t* rowptr_out,
                      int32_t* src_out, int32_t* dst_out, uint32_t* stats, void* workspace, void* stream);

/* -------------------------------------------------------------------------------------------------
 * e3_nl_update_split: the prune above and e3_split_edges in one pass, for the stored graph of a shard's local cloud
 * [owned | ghosts] (sharded_list.ShardedNeighborList).  Open mode only: the local cloud of a shard is an open graph.
 *   inputs  : as e3_nl_update, plus is_ghost [N] uint8 (non-zero = ghost row), in the stored graph's node order.
 *   outputs : pos4_out, rowptr_out, src_out / dst_out as e3_nl_update; src_interior / dst_interior and src_boundary /
 *             dst_boundary (room for E each);  stats [4] uint32 (device), zeroed on the stream inside the entry:
 *             stats[0] = the bits of max_i d2_i over ALL rows, as e3_nl_update;  stats[1] = E_kept = rowptr_out[N];
 *             stats[2] = E_interior;  stats[3] = E_boundary = E_kept - E_interior.
 * Contract: every output is bit for bit what e3_nl_update followed by e3_split_edges (same is_ghost) on its result
 * produces, for any input graph, also one that still has edges into ghost rows:
 *   - a ghost row keeps nothing; an edge of an owned row is kept iff d2 <= fl(r r), the test of e3_nl_update;
 *   - the kept edges go to src_out / dst_out (rowptr_out is their CSR); those with an owned src also to the interior
 *     list, those with a ghost src also to the boundary list;
 *   - every list is in row order and a row's src keep the stored order.
 * One count and one fill pass over the stored edges (a 16-lane group per row, the two ballots "kept" and "kept with a
 * ghost src" give the counts and the write positions) and two exclusive sums; no atomics on the lists.  The composition
 * reads the stored edges twice and the kept edges twice more; this entry reads the stored edges twice and nothing else.
 * E3_ERR_INVALID_ARG as e3_nl_update, and for a NULL is_ghost when N > 0 (the interior / boundary arrays are edge arrays:
 * they may be NULL when E = 0).  N = 0 launches nothing and writes stats = {0, 0, 0, 0} and rowptr_out[0] = 0.
 * workspace = e3_nl_update_split_workspace_bytes(N) bytes (-1 for N outside int32).
 * ------------------------------------------------------------------------------------------------- */
int64_t e3_nl_update_split_workspace_bytes(int64_t N);
int e3_nl_update_split(const float* pos, const int32_t* perm, const float* ref_pos4, const int32_t* rowptr, const int32_t* src,
                       const uint8_t* is_ghost, int64_t N, int64_t E, float r, float* pos4_out, int32_t* rowptr_out,
                       int32_t* src_out, int32_t* dst_out, int32_t* src_interior, int32_t* dst_interior,
                       int32_t* src_boundary, int32_t* dst_boundary, uint32_t* stats, void* workspace, void* stream);

/* =================================================================================================
 * Differentiable ghost refresh of the sharded path (sharding.Halo.refresh / reduce_ghosts): the once-per-layer refresh as
 * an out-of-place row copy, and its backward as a row sum.  Rows are [n, D] of dtype E3_F32 or E3_F64 with a leading
 * dimension (elements); n = the rows of the local cloud [owned | ghosts] in graph order.
 *   slot [n] int32 : -1 for an owned row, else the row's position in the received buffer.
 *   e3_halo_refresh : out[i] = slot[i] < 0 ? h[i] : recv[slot[i]]          (recv [n_recv, D]; h is not written and its
 *             ghost rows are not read; a slot >= n_recv reads nothing and writes a zero row)
 *   e3_halo_reduce  : out[i] = (slot[i] < 0 ? g[i] : 0) + sum_{q = red_ptr[i]}^{red_ptr[i+1] - 1} back[red_k[q]]
 *             back [n_back, D]: the gradient rows that came back for the rows this rank sent, in send order; red_ptr [n + 1]
 *             / red_k [n_back] int32: the send list grouped by its target row (CSR), k ascending inside a row.  The sum
 *             starts from the row's own gradient and adds the list in its order, in the rows' dtype: no atomics, bit-equal
 *             from run to run.  List bounds are clamped to [0, n_back] and a k outside [0, n_back) adds nothing.
 * One wave per row; 16-byte accesses when every pointer is 16-byte aligned and every leading dimension is a multiple of 16
 * bytes, the columns past the last whole 16 bytes (or all, otherwise) by 4- / 8-byte ones: same values either way.
 * E3_ERR_INVALID_ARG before any launch for n < 0, n_recv / n_back < 0, D < 1, a leading dimension below D, a dtype other
 * than E3_F32 / E3_F64, and, when n > 0, a NULL h / g, slot or out, or a NULL recv (back, red_ptr, red_k) with n_recv
 * (n_back) > 0.  n = 0 returns E3_OK and launches nothing; n_recv = 0 / n_back = 0 (no ghosts / nothing sent) are valid.
 * ================================================================================================= */
int e3_halo_refresh(const void* h, int64_t ld_h, const void* recv, int64_t ld_recv, int64_t n_recv, const int32_t* slot,
                    int64_t n, int D, int dtype, void* out, int64_t ld_out, void* stream);
int e3_halo_reduce(const void* g, int64_t ld_g, const void* back, int64_t ld_back, int64_t n_back, const int32_t* slot,
                   const int32_t* red_ptr, const int32_t* red_k, int64_t n, int D, int dtype, void* out, int64_t ld_out,
                   void* stream);

/* =================================================================================================
 * Image rows: periodic cells below twice the cutoff (cell_images.CellImages).  The cloud is extended by explicit lattice
 * images and the graph over [owned (wrapped) | images] is built OPEN (e3_rg_sort_count), so every open edge-stage kernel
 * serves a cell of any size; an image row is refreshed from its owner before every layer and its gradient returns to it.
 * cell / origin / frac / shift / wrap: "General (triclinic) periodic cell" above.  No contraction in any fp32 operation.
 *
 * Selection.  rho = r + 2^-18 (r + sum_k |cell[k]| + sum_a |origin[a]|), evaluated in fp64 in that order and rounded UP to
 *   fp32; shells m_a = max(1, ceil(rho / h_a)) (fp64 quotient of the fp32 values; rho, not r: a wrapped fraction that rounding
 *   left at 1 then cannot need shell m_a + 1).  e3_cell_images_plan (host only) returns both, the shells as they are (capped
 *   at 2^20) so that a caller can name the limit; more than E3_CELL_IMAGE_MAX_SHELLS on an axis is E3_ERR_INVALID_ARG in
 *   count / fill.
 *   For a particle with wrapped position w and s = frac(fl(w - origin)), the shift n != 0, n_a in [-m_a, m_a], is kept iff on
 *   every axis   fl(fl(s_a + n_a) h_a) >= -rho   and   fl(fl(fl(s_a + n_a) - 1) h_a) <= rho:
 *   the image's cell lies within rho of the home cell along the normal of each face pair.  This is a superset of the images
 *   an edge can use (an edge needs |d| <= r, hence at most r along every normal); the edge test stays the graph builder's.
 *   Margin, in ulp (2^-24) of a length: s_a h_a carries 7 roundings (the subtraction, three products, two sums, the rounding
 *   of G) of terms bounded by |w - origin| <= sum |cell[k]|; the test's sum, difference and two products are 3 roundings of
 *   values up to |s_a + n_a| h_a <= 8 h_a, i.e. 24 of h_a <= sum |cell[k]|; the image position fl(w + n cell) carries 4 of a
 *   coordinate of at most |origin| + 8 sum |cell[k]|, i.e. 32 of sum |cell[k]| and 4 of |origin|; the builder's d2 2 of r.
 *   Together 63 of sum |cell[k]|, 4 of sum |origin[a]| and 2 of r: below 64 ulp = 2^-18 of their sum, which grows with the
 *   cell.
 *   e3_cell_images_count : pos [N,3] (may be unwrapped) -> pos_wrapped [N,3] and offsets [N + 1] int32, the exclusive scan
 *             of the per-particle image counts; offsets[N] = G is the ONE value the host reads.  workspace >=
 *             e3_cell_images_workspace_bytes(N) (-1 for N outside [0, 2^31 - 1)).
 *   e3_cell_images_fill  : owner [G] int32, shift [G,3] int32 and image_pos [G,3] = shift(w_owner, -n) = fl(w + n cell),
 *             ordered by (owner ascending, shift lexicographic with n_0 most significant): deterministic, no atomics.
 *             Same cell / origin / r as the count; a particle writes inside [offsets[i], min(offsets[i+1], G)) only.
 *   E3_ERR_INVALID_ARG before any launch for a cell that does not derive, a non-finite origin, r not finite or <= 0,
 *   N (2 m_0 + 1)(2 m_1 + 1)(2 m_2 + 1) >= 2^31 - 1 (so N + G fits int32), N + G >= 2^31 - 1, a short workspace or a NULL
 *   pointer that is needed.  N = 0 is valid: offsets[0] = 0, nothing else is touched.
 *
 * Batches (cell_images.BatchedCellImages): B structures, each with its own cell and origin, one r; structure [N] int32 names
 *   every particle's structure, in any order.  The rule, the rounding and the output order are those above with the cell
 *   looked up per particle -- the particles of one structure get, bit for bit, what the single entries give that structure
 *   alone -- so the images come out by (owner ascending in the caller's order, shift lexicographic), whatever the structures.
 *   e3_cell_images_plan_batch (host only): cells [B,9], origins [B,3] -> shells [B,3] and rho [B] exactly as
 *             e3_cell_images_plan per structure (shells as they are), and table: B records of
 *             e3_cell_images_record_bytes() = E3_CELL_IMAGE_RECORD_BYTES bytes each, a multiple of 16 (cell, inverse, origin,
 *             heights, shells, rho as the kernels hold them; opaque to the caller), in 16-byte aligned HOST memory.  The caller
 *             copies the table to the device, 16-byte aligned, and passes both: the device copy is what the kernels read (one
 *             thread per particle, the record in 16-byte loads), the host copy is what the entries check.
 *   e3_cell_images_count_batch / _fill_batch: as the single pair.  counts [B] int64 (host): the particles of every structure;
 *             a structure without particles is valid.  A particle whose id lies outside [0, B) gets no image and keeps its
 *             position unwrapped (the host layer refuses such input).
 *   E3_ERR_INVALID_ARG before any launch for B outside [0, 2^31 - 1), a structure the single plan refuses, more than
 *   E3_CELL_IMAGE_MAX_SHELLS shells in any structure, a negative count, counts that do not sum to N,
 *   sum_b counts[b] (2 m_0 + 1)(2 m_1 + 1)(2 m_2 + 1) >= 2^31 - 1 with each structure's own shells, N + G >= 2^31 - 1, a table
 *   that is not 16-byte aligned, a short workspace (e3_cell_images_workspace_bytes(N), as above) or a NULL pointer that is
 *   needed.  N = 0 is valid as above.
 *
 * Rows [M, D] with a leading dimension (elements), in any numbering; source [M] int32: source[i] = i on an owned row, the
 * owner's row on an image row (an image row is never a source).
 *   e3_image_rows_expand : out[i] = in[source[i]]; dtype E3_F32, E3_BF16 or E3_F64 (a byte copy).  A source outside [0, M)
 *             writes a zero row.  out == in (same leading dimension) is the in-place form: only the rows with
 *             source[i] != i are written.  shift [M,3] int32 with cell (both or neither; D = 3 and E3_F32 only):
 *             out[i] = shift(in[source[i]], -shift[i]) = fl(in[source[i]] + n_i cell), the positions of the extended cloud.
 *   e3_image_rows_reduce : the transpose.  out[i] = source[i] == i ? g[i] + sum_{q = ptr[i]}^{ptr[i+1] - 1} g[rows[q]] : 0;
 *             ptr [M + 1] / rows [n_rows] int32: the image rows grouped by owner (CSR), ascending inside a row.  The sum
 *             starts from the row's own value and adds the list in its order, in the rows' dtype (E3_F32 or E3_F64): no
 *             atomics, bit-equal from run to run.  List bounds are clamped to [0, n_rows]; a row id outside [0, M) adds
 *             nothing.  out must not be g.
 *   One wave per row; 16-byte accesses when every pointer is 16-byte aligned and every leading dimension is a multiple of 16
 *   bytes, the remaining columns (or all) element by element: same values either way.  E3_ERR_INVALID_ARG before any launch
 *   for M outside [0, 2^31 - 1), D < 1, a leading dimension below D, another dtype, a shift without a cell (or the reverse,
 *   or with D != 3 / another dtype), an in-place call with two leading dimensions, and, when M > 0, a NULL pointer that is
 *   needed.  M = 0 returns E3_OK and launches nothing.
 * ================================================================================================= */
#define E3_CELL_IMAGE_MAX_SHELLS 7
int e3_cell_images_plan(const float cell[9], const float origin[3], float r, int32_t shells[3], float* rho);  /* host only */
int64_t e3_cell_images_workspace_bytes(int64_t N);
int e3_cell_images_count(const float* pos, int64_t N, const float cell[9], const float origin[3], float r, float* pos_wrapped,
                         int32_t* offsets, void* workspace, int64_t workspace_bytes, void* stream);
int e3_cell_images_fill(const float* pos_wrapped, int64_t N, const float cell[9], const float origin[3], float r,
                        const int32_t* offsets, int64_t G, int32_t* owner, int32_t* shift, float* image_pos, void* stream);
#define E3_CELL_IMAGE_RECORD_BYTES 112
int64_t e3_cell_images_record_bytes(void);
int e3_cell_images_plan_batch(const float* cells, const float* origins, int64_t B, float r, int32_t* shells, float* rho,
                              void* table);  /* host only */
int e3_cell_images_count_batch(const float* pos, const int32_t* structure, int64_t N, const void* table,
                               const void* table_host, const int64_t* counts, int64_t B, float* pos_wrapped, int32_t* offsets,
                               void* workspace, int64_t workspace_bytes, void* stream);
int e3_cell_images_fill_batch(const float* pos_wrapped, const int32_t* structure, int64_t N, const void* table,
                              const void* table_host, const int64_t* counts, int64_t B, const int32_t* offsets, int64_t G,
                              int32_t* owner, int32_t* shift, float* image_pos, void* stream);
int e3_image_rows_expand(const void* in, int64_t ld_in, const int32_t* source, const int32_t* shift, const float cell[9],
                         int64_t M, int D, int dtype, void* out, int64_t ld_out, void* stream);
int e3_image_rows_reduce(const void* g, int64_t ld_g, const int32_t* source, const int32_t* ptr, const int32_t* rows,
                         int64_t n_rows, int64_t M, int D, int dtype, void* out, int64_t ld_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* E3GNN_H */
