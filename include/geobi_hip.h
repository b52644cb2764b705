/* libgeobi_hip.so -- C ABI of the MI355X-native bi-domain mesh-graph convolution path.
 *
 * The reference (zhangyk18/GeoBi-GNN) has no FFI layer: its "operator API" for this path is the
 * Python nn.Module surface (code/network.py:254-343, code/net_util.py:56-380) over third-party
 * PyTorch extensions.  Each entry point below replaces the native kernel(s) one of those call
 * sites dispatches to; the replaced call site is cited per function.  INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a BORROWED device pointer (HBM) unless marked `host`; the library never
 *     allocates, frees or synchronises: scratch comes in through `ws` / `ws_bytes` (query the size
 *     with the matching *_ws_bytes function, which is a pure host computation + rocPRIM size query).
 *     Documented exceptions (plus one helper): geobi_read_i32 (the size read-back: waits for `stream`), geobi_clean_faces
 *     (reads its undecided counts through it), geobi_topo_orient / _components / _report (read the changed flags of
 *     their rounds through it), geobi_subdiv_plan, geobi_decim_plan, geobi_decim_plan_short, geobi_flip_plan, geobi_relax,
 *     geobi_move_to and geobi_fill_plan with stage_ms (wait for their own end; without it the call is only enqueued and the caller reads its counts through geobi_read_i32, once per pass), the whole-network
 *     entry points geobi_net_forward / geobi_net_forward_train / geobi_net_train_groups (four reads of pooling sizes
 *     per pass, through mapped host memory) -- and, for its own purpose, geobi_host_mailbox (hands out mapped HOST memory)
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*)
 *   - return value 0 = ok, non-zero = error; the message is in geobi_last_error() (thread-local)
 *   - node features are row-major fp32; indices inside the library are int32.  Per call and graph level at most
 *     GEOBI_MAX_NODES nodes (rows of any per-node array, faces and vertices alike) and GEOBI_MAX_EDGES edges: below
 *     these every 32-bit element index a kernel forms -- node x channels (<= 128), node x 16 lanes, edge x 16 lanes --
 *     stays under 2^31 / 2^32; byte and float offsets into per-node / per-edge rows are 64-bit throughout.  Larger
 *     sizes are REJECTED by the entry points (error code, message), never truncated.  The path's largest
 *     configuration (a 150 k-face scan: 1.97 M edges) is 1 % of the limits; bigger meshes go through the patch split.
 *     The reference's int64 COO `edge_index` is accepted by geobi_csr_from_coo
 *   - FeaSt heads are fixed at 9 (every FeaStConv on the path is built with heads=9,
 *     code/network.py:258-268); per-node / per-edge head vectors use a padded row stride of
 *     GEOBI_HEAD_STRIDE floats
 */
#ifndef GEOBI_HIP_H_
#define GEOBI_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GEOBI_HEADS 9
#define GEOBI_HEAD_STRIDE 12
#define GEOBI_MAX_NODES ((1 << 24) - 1)  /* 16 777 215 */
#define GEOBI_MAX_EDGES ((1 << 28) - 1)  /* 268 435 455 */

int geobi_version(void);
const char* geobi_last_error(void);

/* ---------------------------------------------------------------- adjacency (CSR) ----------
 * Replaces the per-call COO handling inside torch_geometric.MessagePassing / remove_self_loops /
 * add_self_loops (FeaStConv.forward, called at code/network.py:271-299) and the CSR build inside
 * torch_cluster.graclus (code/net_util.py:127).
 *
 * geobi_csr_from_coo: sort E (segment, neighbour) int64 pairs by (segment, neighbour); self loops
 * are dropped when drop_self != 0.  rowptr[N] is the number of kept edges; col / eid have E slots
 * (eid[k] = position of sorted edge k in the input COO).  Pairs with an id outside [0, N) are dropped
 * and counted in bad[0] (device int32, optional): they never reach a kernel as an index.
 * The sort is stable: eid ascends within a run of equal pairs.  Beyond rowptr[N], col is -1 and eid lists the dropped
 * pairs in input order, so eid as a whole is a permutation of 0 .. E-1.
 * geobi_csr_transpose: CSR of the reversed edges; pos_t[e'] = index of that edge in the input CSR,
 * inv_pos[e] = index of input edge e in the transposed CSR (inv_pos may be NULL, pos_t may not).  The valid edge count is
 * read on the device (rowptr[N], which must not exceed Ecap, the length of col / col_t / pos_t); equal edges keep their
 * input order; col_t and pos_t are -1 in [rowptr[N], Ecap) and inv_pos is written only below rowptr[N]. */
size_t geobi_csr_ws_bytes(int64_t E, int64_t N);
int geobi_csr_from_coo(const int64_t* seg, const int64_t* nbr, int64_t E, int64_t N, int drop_self,
                       int32_t* rowptr, int32_t* col, int32_t* eid, int32_t* bad, void* ws, size_t ws_bytes,
                       void* stream);
int geobi_csr_transpose(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t Ecap, int32_t* rowptr_t,
                        int32_t* col_t, int32_t* pos_t, int32_t* inv_pos, void* ws, size_t ws_bytes, void* stream);
/* geobi_csr_reverse_index: for a (row, col)-sorted CSR, pos_rev[e] = position of the reverse of edge e
 * (or -1, with flag[0] |= 1, when it is missing; flag is zeroed first and may be NULL when the caller
 * already knows the graph is symmetric).  Where the reverse edge is listed several times it is the FIRST of that run, for
 * every copy of e: on a multigraph pos_rev is no permutation.  For a symmetric graph (every mesh graph of the
 * path, and every pooled graph derived from one) the transposed CSR equals the CSR and pos_rev is the
 * edge correspondence -- no second sort. */
int geobi_csr_reverse_index(const int32_t* rowptr, const int32_t* row, const int32_t* col, int64_t E,
                            int32_t* pos_rev, int32_t* flag, void* stream);
int geobi_expand_rowptr(const int32_t* rowptr, int64_t N, int32_t* row, void* stream);
int geobi_gather_f32(const float* src, const int32_t* idx, int64_t n, float* dst, void* stream);
/* geobi_concat32: the disjoint-union batch of several meshes (the data loader's collate step: code/train_dual.py:199-201
 * hands the meshes over one by one; a batch is their union) as ONE launch per element type instead of a cat + add per
 * array and mesh.  `segs` is a HOST array of n_segs copy jobs over 4-byte elements:
 *   dst[i] = src[i] + add      (is_float == 0: int32 -- row pointers shifted by the edge offset, neighbour / vertex ids by
 *                               the node offset, reverse-edge and corner positions by theirs)
 *   dst[i] = src[i]            (is_float != 0: features, targets, weights; `add` ignored)
 *   src == NULL: dst[i] = add  (int32) / value (float): closing row pointers, constant per-mesh loss weights.          */
typedef struct {
  const void* src;
  void* dst;
  int64_t n;
  int32_t add;
  float value;
} geobi_copy_seg_t;
int geobi_concat32(const geobi_copy_seg_t* segs, int n_segs, int is_float, void* stream);

/* ---------------------------------------------------------------- FeaSt convolution --------
 * Replaces torch_geometric.nn.FeaStConv.forward / its autograd (16 call sites,
 * code/network.py:271,279,286,287,290,293,296,299), optionally fused with the leaky_relu that
 * follows most of them (slope = 1 disables it) and with the skip concatenation of
 * code/network.py:292,298 (the input may be given as two equal halves xa | xb; Cb = 0 otherwise).
 *
 *   in-CSR  : rowptr_in/col_in   -- for every TARGET node its SOURCE nodes (edge_index[0] -> [1])
 *   out-CSR : rowptr_out/col_out -- for every SOURCE node its TARGET nodes; pos_in[e] = position of
 *             out-edge e in the in-CSR.  Both without self loops (one per node is implied).
 *   lin_w [9*Cout, Cin], u_w [9, Cin], c [9], bias [Cout]   (PyG >= 2.0 state-dict layout)
 *   forward saves p [N, 12] (x u^T; not written for unsplit 6- / 12-channel inputs, whose logits are formed
 *   per edge from the rows themselves) for the backward; `out` after the activation is needed by the backward
 *   when slope != 1.
 *   z == NULL (the default of the Python layer): FUSED path -- aggregation and node transform in one kernel, the
 *   aggregated features [N, 9 Cin] stay in LDS and never reach HBM; the backward (z == NULL as well) recomputes
 *   them and forms dx in a second fused kernel.  z != NULL: [N, geobi_feast_ldz(Cin)] receives the aggregated
 *   features (separate aggregation + GEMM kernels) and must be handed to the backward.
 *   wf (optional, geobi_feast_wpack_floats(Cin, Cout) floats) receives the packed weights -- Wf [ldz, Cout],
 *   W' = [lin.weight ; u.weight ; 0] [9 Cout + 24, Cin], then the MFMA-fragment-ordered forms of both that the
 *   fused kernels read -- in the forward and, handed back to the backward, saves repacking them there (NULL:
 *   packed into the workspace on both sides).
 *   E = number of edges in the CSR (used for scratch sizing and byte accounting only).
 *   Supported channel counts: Cin, Cout in {6, 12, 32, 64, 128} (Cout: 32, 64, 128).           */
int geobi_feast_ldz(int Cin);
size_t geobi_feast_wpack_floats(int Cin, int Cout);
size_t geobi_feast_fwd_ws_bytes(int64_t N, int Cin, int Cout);
int geobi_feast_fwd(const float* xa, const float* xb, int Ca, int Cb, int64_t N, int64_t E,
                    const int32_t* rowptr_in, const int32_t* col_in, const float* lin_w, const float* u_w,
                    const float* c, const float* bias, int Cout, float slope, float* out, float* p, float* z,
                    float* wf, void* ws, size_t ws_bytes, void* stream);
size_t geobi_feast_bwd_ws_bytes(int64_t N, int64_t E, int Cin, int Cout);
/* dxa/dxb may be NULL (input needs no gradient); dlin_w/du_w/dc/dbias are overwritten, or added to when
 * accumulate != 0 (a caller that lets the kernels write into persistent .grad storage: gradient accumulation
 * over several backward passes, code/train_dual.py:211-218). */
int geobi_feast_bwd(const float* xa, const float* xb, int Ca, int Cb, int64_t N, int64_t E,
                    const int32_t* rowptr_in, const int32_t* col_in, const int32_t* rowptr_out,
                    const int32_t* col_out, const int32_t* pos_in, const float* lin_w, const float* u_w,
                    const float* c, int Cout, float slope, const float* out, const float* gout, const float* p,
                    const float* z, const float* wf, float* dxa, float* dxb, float* dlin_w, float* du_w, float* dc,
                    float* dbias, int accumulate, void* ws, size_t ws_bytes, void* stream);

/* Tile geometry of the fused FeaSt kernels: 16 (default: 16-node tiles on v_mfma_f32_16x16x4_f32, four workgroups per
 * CU) or 32 (round-2 geometry: v_mfma_f32_32x32x2_f32, two per CU); 0 returns to the GEOBI_TILE16 environment default.
 * Process-wide; for parity tests and same-process A/B timing.                                                       */
int geobi_set_tile_rows(int rows);

/* Form of the fused backward row pass of layers reading 64 channels; each argument 1, 0 or -1 (= default).
 * staged (default 1, GEOBI_ROWPASS_STAGED): the neighbour rows reach the lane = edge dot products through LDS
 *   (global_load_lds_dwordx4, half a row per eight lanes) instead of sixteen private 16-B reads per lane; bit-identical.
 * chunked64 (default: Cout = 128 only, GEOBI_ROWPASS_CHUNKED64): the channel-chunked kernel of the 128-channel layers
 *   (32-node tiles, 32 channels at a time) instead of the 16-node-tile kernel.
 * Process-wide; for parity tests and same-process A/B timing.                                                       */
int geobi_set_rowpass_form(int staged, int chunked64);
/* column parts of the fused FeaSt kernel (16-row tiles, layers reading 128 channels): 2 = every tile is worked on by two
 * workgroups, each producing half of the output columns; 1 = off; 0 = chosen per launch from the tile count (default: two parts
 * up to 512 tiles; GEOBI_COLUMN_PARTS, GEOBI_COLUMN_PARTS_MAX_TILES).  Bit-identical results. */
int geobi_set_column_parts(int parts);

/* ---------------------------------------------------------------- pooling ------------------
 * geobi_edge_weight_t10 : PoolingLayer._get_edge_weight, edge_weight_type 10
 *                         (code/net_util.py:226-230):  w_out = w_in + exp(-|x_row - x_col|^2 / 2)
 * geobi_match_heavy_edge: torch_cluster.graclus (code/net_util.py:127,325,353): heavy-edge matching,
 *                         cluster[u] = cluster[v] = min(u, v), unmatched -> own id.  Deterministic
 *                         (greedy in descending edge order).  init != 0 starts from scratch, init == 0
 *                         continues from `cluster` (the resumable state: -1 undecided, u closed as a
 *                         singleton, v matched with partner v); status[0] = nodes still undecided
 *                         after `rounds` proposal rounds (0 = converged); cluster_final (optional)
 *                         receives a copy with the undecided nodes closed as singletons.
 * geobi_relabel_compact : torch_geometric consecutive_cluster (code/net_util.py:128): dense ids by
 *                         ascending cluster id; count[0] = number of clusters (device int32).
 *                         rep_is_self != 0: the caller guarantees that every cluster id is the index of
 *                         one of its own members with cluster[id] == id (true for graclus / the matching
 *                         above: id = min member) -- saves the occupancy pass.
 * geobi_segment_csr     : inverse lists segment -> members (ascending), the sorted-segment form of
 *                         torch_scatter's index argument.
 * geobi_segment_max_*   : torch_scatter.scatter(reduce='max') + backward (code/net_util.py:134);
 *                         first maximum wins, empty segments give 0.
 * geobi_segment_sum     : scatter(reduce='sum'|'mean') forward (code/net_util.py:132) and the
 *                         backward of the unpool gather `x[unpooling_indices]` (:242-245).
 * geobi_gather_rows     : PoolingLayer.unpooling forward (code/net_util.py:242-245).
 * geobi_pool_edge       : pool_edge (code/net_util.py:289-295): relabel endpoints, drop loops,
 *                         sort by (row, col), merge duplicates (mean of weights).  Outputs sized for
 *                         E entries / nmax+1 row pointers; count[0] = kept edges (device int32).   */
int geobi_edge_weight_t10(const float* x, int C, const int32_t* row, const int32_t* col, const float* w_in,
                          int64_t E, float* w_out, void* stream);
/* geobi_edge_weight_att: PoolingLayer._get_edge_weight, edge_weight_type 3 / 4 / 5 (code/net_util.py:182-206): the
 * GAT-style learned weight  sigmoid((al[row] + ar[col]) + (al[col] + ar[row])),  al = x . att_l,  ar = x . att_r  per node
 * (x [N, C]: the features for type 3, leaky_relu(lin(x), 0.2) for types 4 / 5 -- geobi_gemm_nn with bias and slope);
 * w_in != NULL: averaged with the given weight, (sigmoid + w_in) / 2 (type 5).  node_ws: 2 N floats of scratch.          */
int geobi_edge_weight_att(const float* x, int C, const float* att_l, const float* att_r, const int32_t* row,
                          const int32_t* col, const float* w_in, int64_t N, int64_t E, float* node_ws, float* w_out,
                          void* stream);
size_t geobi_match_ws_bytes(int64_t N);
int geobi_match_heavy_edge(const int32_t* rowptr, const int32_t* col, const float* w, int64_t N, int rounds,
                           int init, int32_t* cluster, int32_t* cluster_final, int32_t* status, void* ws, size_t ws_bytes, void* stream);
/* test hook: at most cap x (rounds / 8) proposal rounds per call (<= 0: no cap).  With cap = 1 the default 8 rounds
 * become 1 and every resume of a caller's repair loop (rounds doubled each time) 2, 4, ...: the resume paths of
 * PoolingLayer.forward / geobi_net_forward run on graphs that otherwise converge at once. */
int geobi_set_match_round_cap(int cap);
/* test hooks for the forms of the pooling front end (1 / 0 force a form, a negative value goes back to what the
 * environment variable of the same knob says; results do not depend on the form):
 *   geobi_set_match_scanfree: geobi_match_coarsen's tail -- the scan-free kernel pair (default up to 2^20 nodes,
 *                             GEOBI_MATCH_SCANFREE) or commit + exclusive scans + lists
 *   geobi_set_scan_lookback : the exclusive int scan of 2^14 < n <= 2^18 entries -- the several-block look-back kernel
 *                             (default, GEOBI_SCAN_LOOKBACK) or the one-block walk                                  */
int geobi_set_match_scanfree(int on);
int geobi_set_scan_lookback(int on);
/* geobi_match_coarsen: the integer front end of one pooling step (code/net_util.py:127-128 plus the inverse
 * lists the feature pooling needs) in one call: the rounds of geobi_match_heavy_edge, then dense ids and
 * segment lists of the matching -- the results of geobi_relabel_compact and geobi_segment_csr_pairs, with
 * 6 launches fewer.  state [N]: resumable (-1 undecided, u singleton, v partner); cluster_final [N]: graclus
 * ids (min member; undecided nodes closed as singletons); cnew [N]; segptr [N+1], members [N] (sized by the
 * fine node count); counters[0] = undecided nodes, counters[1] = coarse node count (device int32).        */
size_t geobi_match_coarsen_ws_bytes(int64_t N);
int geobi_match_coarsen(const int32_t* rowptr, const int32_t* col, const float* w, int64_t N, int rounds, int init,
                        int32_t* state, int32_t* cluster_final, int32_t* cnew, int32_t* segptr, int32_t* members,
                        int32_t* counters, void* ws, size_t ws_bytes, void* stream);
size_t geobi_relabel_ws_bytes(int64_t N);
int geobi_relabel_compact(const int32_t* cluster, int64_t N, int rep_is_self, int32_t* cnew, int32_t* count,
                          void* ws, size_t ws_bytes, void* stream);
size_t geobi_segment_csr_ws_bytes(int64_t n);
int geobi_segment_csr(const int32_t* seg, int64_t n, int64_t nseg, int32_t* segptr, int32_t* members, void* ws,
                      size_t ws_bytes, void* stream);
/* Sort-free inverse lists: _pairs for a matching (clusters of <= 2 nodes, raw id = smaller member, as
 * graclus / geobi_match_heavy_edge emit, cnew = its dense relabelling); _compose for the lists of a
 * composed index fine -> mid -> coarse (the `clust2[clust1]` of code/net_util.py:152-156). */
size_t geobi_segment_pairs_ws_bytes(int64_t nseg);
int geobi_segment_csr_pairs(const int32_t* cnew, const int32_t* raw, int64_t N, int64_t nseg, int32_t* segptr,
                            int32_t* members, void* ws, size_t ws_bytes, void* stream);
int geobi_segment_csr_compose(const int32_t* segptr1, const int32_t* members1, const int32_t* segptr2,
                              const int32_t* members2, int64_t nseg2, int64_t n_fine, int32_t* segptr12,
                              int32_t* members12, void* ws, size_t ws_bytes, void* stream);
int geobi_segment_max_fwd(const float* x, int C, const int32_t* segptr, const int32_t* members, int64_t nseg,
                          float* out, int32_t* arg, void* stream);
int geobi_segment_max_bwd(const float* gout, const int32_t* arg, const int32_t* seg, int C, int64_t nseg,
                          int64_t n_fine, float* gx, void* stream);
int geobi_segment_sum(const float* x, int C, const int32_t* segptr, const int32_t* members, int64_t nseg, int mean,
                      float* out, void* stream);
int geobi_segment_mean_bwd(const float* gout, const int32_t* seg, const int32_t* segptr, int C, int64_t n_fine,
                           float* gx, void* stream);
int geobi_gather_rows(const float* x, const int32_t* idx, int C, int64_t n_out, float* out, void* stream);
/* Sort-free pool_edge for a MATCHING: one wave per coarse node merges the (at most two) fine rows of its
 * members with a 64-lane bitonic network.  (segptr, members) = geobi_segment_csr_pairs built with
 * nseg = nbound = fine node count; ncount = device count of coarse nodes (geobi_relabel_compact).
 * overflow[0] |= 1 when a coarse node gathers more than 64 fine entries: use geobi_pool_edge then. */
size_t geobi_pool_edge_rows_ws_bytes(int64_t nbound);
int geobi_pool_edge_rows(const int32_t* cnew, const int32_t* segptr, const int32_t* members, const int32_t* rowptr,
                         const int32_t* col, const float* w, const int32_t* ncount, int64_t nbound,
                         int32_t* rowptr_c, int32_t* row_c, int32_t* col_c, float* w_c, int32_t* count,
                         int32_t* overflow, void* ws, size_t ws_bytes, void* stream);
size_t geobi_pool_edge_ws_bytes(int64_t E);
int geobi_pool_edge(const int32_t* cnew, const int32_t* row, const int32_t* col, const float* w, int64_t E,
                    int64_t nmax, int32_t* rowptr_c, int32_t* row_c, int32_t* col_c, float* w_c, int32_t* count,
                    void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- geometry coupling --------
 * DualGNN.forward, code/network.py:335-337 + data_util.computer_face_normal (code/data_util.py:182-198):
 * out[f] = (xf[f, 0:6], centroid of the predicted triangle, its unit normal).  The backward emits
 * per-corner gradients [3F, 3] which geobi_segment_sum folds into the vertices through the
 * vertex -> corner inverse lists.                                                               */
int geobi_face_geom_fwd(const float* verts, const int32_t* fv, const float* xf, int ldxf, int64_t F, float* out,
                        void* stream);
int geobi_face_geom_bwd(const float* verts, const int32_t* fv, const float* gout, int64_t F, float* corner_grad,
                        void* stream);

/* ---------------------------------------------------------------- heads --------------------
 * code/network.py:324-332 (vertex head, mode 0: fc2(lrelu(fc1 x)) (* depth_direction) + xyz) and
 * :340-343 (face head, mode 1: F.normalize(fc2(lrelu(fc1 x)), dim=1)).  raw [N,nout] is saved for the
 * backward.  h = NULL selects the fused kernels (Cin = 32, K = 1024): the [N, K] hidden activation
 * stays in the matrix-core accumulators, forward and backward (recomputed), and never reaches HBM;
 * with a non-NULL h [N,K] the hidden activation is materialised and the generic GEMMs are used.   */
int geobi_head_fwd(const float* x, int Cin, int64_t N, const float* w1, const float* b1, int K, const float* w2,
                   const float* b2, int nout, float slope, int mode, const float* dd, const float* resid,
                   int ld_resid, float* h, float* raw, float* out, void* stream);
/* Precision of the heads' 32 -> 1024 product (process-wide switch, default 0; GEOBI_HEAD_BF16X3=1 starts with 1):
 *   0  exact fp32 on v_mfma_f32_32x32x2_f32 -- what every number of the bench line and every parity test uses
 *   1  the same product as SIX bf16 products with fp32 accumulation (each operand cut into three bf16 pieces: 24 significand
 *      bits; v_mfma_f32_32x32x16_bf16, 16 x the fp32 matrix rate): not bit-identical to mode 0, but no farther from fp64 than
 *      mode 0 is on the path's operands (profiles/r04_bf16_split_study.txt, test_head_split_precision_*).  A labelled variant:
 *      the reference computes in fp32 (code/network.py:324-343).                                                          */
int geobi_set_head_precision(int mode);
size_t geobi_head_bwd_ws_bytes(int64_t N, int Cin, int K);
int geobi_head_bwd(const float* x, int Cin, int64_t N, const float* w1, const float* b1, int K, const float* w2,
                   int nout, float slope, int mode, const float* dd, const float* h, const float* raw, const float* gout,
                   float* dx, float* dw1, float* db1, float* dw2, float* db2, int accumulate, void* ws,
                   size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- losses / metrics ---------
 * code/network.py:364-413 on [n, 3] rows:  out[0] = scale * sum_i w_i * term_i  (w = NULL: w_i = 1)
 *   kind 0  L1   sum_c |a - b|          (loss_v / loss_n 'L1')       kind 1  L2  sum_c (a - b)^2
 *   kind 2  Euclidean distance          (error_v)                    kind 3  angle in degrees (error_n)
 * scale = 1/n gives the reference's `.mean()`; per-row weights give per-mesh means of a batch.
 * Deterministic two-stage reduction.  _bwd (kinds 0, 1): ga = gout[0] * scale * w_i * d term / d a.  */
size_t geobi_row_loss_ws_bytes(int64_t n);
int geobi_row_loss_fwd(const float* a, const float* b, const float* w, int64_t n, int kind, float scale, float* out,
                       void* ws, size_t ws_bytes, void* stream);
int geobi_row_loss_bwd(const float* a, const float* b, const float* w, const float* gout, int64_t n, int kind,
                       float scale, float* ga, void* stream);

/* ---------------------------------------------------------------- nearest distances (evaluation) ----
 * The vertex metric of the denoising evaluation, data_util.eval_denoising_result (code/data_util.py:559-638), by brute
 * force over all pairs: exact, deterministic (no atomics), fp32 with every pair's squared distance formed from coordinate
 * DIFFERENCES (translation-invariant; no |q|^2 + |t|^2 - 2 q.t cancellation), one sqrt per query.  Among equally near
 * targets the LOWEST index is returned.  The targets are cut into slices so that small query sets fill the chip
 * (geobi_nearest_slices: how many the library picks for the sizes -- a pure host function); the results are bit-identical
 * for every slice count.  A query with a NaN coordinate gets dist = +inf.
 *   geobi_nearest_point     my_hausdorff.nearest_distance(XA, XB, 'euclidean') (code/data_util.py:604, code/my_hausdorff.py):
 *                           dist[i] = min_j |q_i - t_j|, idx[i] = that j (idx may be NULL)
 *   geobi_nearest_triangle  the point-to-surface form the reference keeps commented out beside it (p2m,
 *                           code/data_util.py:601-603): distance from q_i to the closest point -- interior, edge or corner --
 *                           of the closest triangle of (verts [V,3], fv [F,3]); face[i] = that triangle (may be NULL).
 *                           Triangles without area count as their longest edge.  fv must index [0, V): range-check it
 *                           first (the Python layer does; the kernel clamps what it reads, it does not report)
 *   geobi_dist_summary      out (DEVICE double[2]) = sum and max of dist [n], accumulated in fp64 in a fixed order: the
 *                           .sum() / .mean() of code/data_util.py:610-616 and the directed Hausdorff maximum
 * ws: geobi_nearest_ws_bytes(Q, T) (T = targets: points or triangles) serves either nearest call.                       */
size_t geobi_nearest_ws_bytes(int64_t Q, int64_t T);
int geobi_nearest_slices(int64_t Q, int64_t T, int triangles);
int geobi_nearest_point(const float* q, const float* t, int64_t Q, int64_t T, float* dist, int32_t* idx, void* ws,
                        size_t ws_bytes, void* stream);
int geobi_nearest_triangle(const float* q, const float* verts, const int32_t* fv, int64_t Q, int64_t V, int64_t F,
                           float* dist, int32_t* face, void* ws, size_t ws_bytes, void* stream);
size_t geobi_dist_summary_ws_bytes(int64_t n);
int geobi_dist_summary(const float* dist, int64_t n, void* out, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- correspondence-free losses ----
 * The two loss options of the reference that need no vertex-to-vertex correspondence: loss_v(vp, v, dis='CD')
 * (code/network.py:369-370, kaolin's chamfer_distance: squared distances, both directions, means) and
 * loss_n(np, n, norm='sided', fc_p, fc) (code/network.py:385-388, kaolin's sided_distance: the index of the nearest
 * ground-truth face centroid), for a disjoint-union batch of P meshes: every search stays inside its own mesh.
 * qptr / tptr [P + 1] are HOST arrays (rows qptr[p] .. qptr[p + 1] of q and tptr[p] .. tptr[p + 1] of t are part p) that
 * travel in the kernel arguments as geobi_rotate_parts' part_ptr does, 32 parts per launch: no copy, no sync.  P >= 1;
 * an EMPTY part on either side is an error; qptr[P] and tptr[P] are bounded by GEOBI_MAX_NODES.
 *   geobi_nearest_parts   d2[i] = min_j |q_i - t_j|^2 over the targets j of i's own part (SQUARED, no sqrt), idx[i] = that j
 *                         as a row of t (the lowest among equally near ones).  Same kernel shape and the same pair
 *                         arithmetic as geobi_nearest_point: for any part, idx - tptr[p] is what geobi_nearest_point
 *                         returns on that part's rows alone (and d2 the square its dist is the root of), whatever the slicing
 *                         (geobi_nearest_parts_slices: the largest slice count the library picks -- a pure host function).
 *                         A query with a NaN coordinate gets d2 = +inf and the first row of its slice range: never an
 *                         index outside its part.  ws: geobi_nearest_parts_ws_bytes(qptr, tptr, P)
 *   geobi_chamfer_fwd     out[0] = sum_p (1/P) [ mean_{i in p} d2a[i] + mean_{j in p} d2b[j] ],  d2a [qptr[P]] / d2b [tptr[P]]
 *                         = geobi_nearest_parts prediction -> target / target -> prediction; fp64 sums in a fixed order.
 *                         ws: geobi_chamfer_ws_bytes(P)
 *   geobi_chamfer_bwd     gp[i] = gout[0] * ( 2 / (P Q_p) (p_i - t_idx_a[i]) + 2 / (P M_p) sum_{j : b(j) = i} (p_i - t_j) ):
 *                         the arg-min maps are constants, the gradient goes to the prediction only.  idx_a [Q]: the
 *                         indices of the first search; (segptr [Q + 1], members [M]) = geobi_segment_csr of the second
 *                         search's indices b with nseg = Q (members ascending).  Every row of gp is written once, no
 *                         atomics; needs qptr[0] == tptr[0] == 0.
 * The sided normal loss needs no arithmetic of its own: geobi_nearest_parts on the face centroids, geobi_gather_rows of
 * the ground-truth normals, geobi_row_loss_* (kind 0) with the per-mesh weights.                                          */
size_t geobi_nearest_parts_ws_bytes(const int64_t* qptr, const int64_t* tptr, int P);
int geobi_nearest_parts_slices(const int64_t* qptr, const int64_t* tptr, int P);
int geobi_nearest_parts(const float* q, const float* t, const int64_t* qptr, const int64_t* tptr, int P, float* d2,
                        int32_t* idx, void* ws, size_t ws_bytes, void* stream);
size_t geobi_chamfer_ws_bytes(int P);
int geobi_chamfer_fwd(const float* d2a, const float* d2b, const int64_t* qptr, const int64_t* tptr, int P, float* out,
                      void* ws, size_t ws_bytes, void* stream);
int geobi_chamfer_bwd(const float* p, const float* t, const int32_t* idx_a, const int32_t* segptr, const int32_t* members,
                      const int64_t* qptr, const int64_t* tptr, int P, const float* gout, float* gp, void* stream);

/* ---------------------------------------------------------------- mesh regularisers ----
 * Two differential terms on the mesh itself, for training without correspondence (Chamfer / sided losses see no
 * connectivity): the reference's laplacian_loss(vp, v, edge_idx_v, normal) (code/network.py:347-361) and an edge-length
 * term.  Both live on the loop-free SYMMETRIC vertex CSR (rowptr [V + 1], col [E], int32, columns ascending in a row) that
 * the prediction vp [V,3] and the ground truth v [V,3] share.  N(i) = row i, deg_i its length, m_i = max(deg_i, 1).
 *   lap(p)_i = (1 / m_i) sum_{j in N(i)} (p_i - p_j);  with normal [V,3] (may be NULL): lap(p)_i <- n_i (n_i . lap(p)_i)
 *   d_i      = lap(vp)_i - lap(v)_i
 *   L_lap    = sum_i w_lap[i] sum_c |d_ic|                                   (network.py:360-361: .abs().sum(1).mean())
 *   L_edge   = sum_i w_edge[i] sum_{j in N(i)} (|vp_i - vp_j| - |v_i - v_j|)^2
 * w_lap / w_edge [V] are per-ROW weights: 1 / (B n_mesh) and 1 / (B E_mesh) give the mean over the B meshes of a union
 * batch of the per-mesh means; NULL: 1 / V and 1 / E (0 when E = 0), the plain means.  terms: bit 0 the Laplacian term,
 * bit 1 the edge term (1, 2 or 3); a term that is off costs nothing and its output is 0.
 *   geobi_mesh_reg_fwd   out[0] = L_lap, out[1] = L_edge: one pass over the rows (a neighbour's two points are gathered once
 *                        for both terms), sums of coordinate differences in ascending column order, fp64 block sums added in
 *                        a fixed order.  With bit 0 it also writes the backward seed u [V,3] (NULL without bit 0):
 *                        u_i = w_lap[i] g_i / m_i,  g_i = sign(d_i), or n_i (n_i . sign(d_i)) with a normal; sign(0) = 0.
 *                        ws: geobi_mesh_reg_ws_bytes(V)
 *   geobi_mesh_reg_bwd   gvp_k = gout[0] (deg_k u_k - sum_{i in N(k)} u_i)
 *                                + gout[1] sum_{j in N(k)} (w_edge[k] + w_edge[j]) 2 (|e_p| - |e_g|) e_p / |e_p|,
 *                        e_p = vp_k - vp_j, e_g = v_k - v_j; an entry with |e_p| = 0 adds nothing.  gout: DEVICE float[2],
 *                        the gradients of the two outputs (the one of a term that is off is not read).  One gather per
 *                        row, every row of gvp written once, no atomics: it relies on k in N(i) <=> i in N(k), so the
 *                        CALLER must know the graph to be symmetric (the Python layer refuses any other).  The gradient
 *                        goes to vp only.
 * Same input, same bits.  What is read through rowptr / col is clamped to the arrays.  V >= 1.                          */
size_t geobi_mesh_reg_ws_bytes(int64_t V);
int geobi_mesh_reg_fwd(const float* vp, const float* v, const float* normal, const int32_t* rowptr, const int32_t* col,
                       int64_t V, int64_t E, const float* w_lap, const float* w_edge, int terms, float* out, float* u,
                       void* ws, size_t ws_bytes, void* stream);
int geobi_mesh_reg_bwd(const float* vp, const float* v, const int32_t* rowptr, const int32_t* col, int64_t V, int64_t E,
                       const float* u, const float* w_edge, const float* gout, int terms, float* gvp, void* stream);

/* ---------------------------------------------------------------- rigid ICP alignment ----
 * Point-to-point ICP of x [Q, 3] onto y [M, 3] per part of a disjoint-union batch (host part pointers as above): what
 * loss_v(..., apply_icp=True) asks of pytorch3d's iterative_closest_point (code/network.py:15,364-367).  The convention is
 * xt = s x R + T with row vectors, det R = +1 unless reflections are allowed.  One iteration is geobi_nearest_parts(xt, y)
 * followed by geobi_icp_step, which aligns the ORIGINAL x to y[idx] by Umeyama's closed form in fp64 (3x3 SVD by one-sided
 * Jacobi: C^T C is never formed), writes xt = float32(s x R + T) rounded once, and takes rmse from the fp64 values.  A part
 * converges at iteration k if k >= 2, prev_rmse > 0 and (prev_rmse - rmse) / prev_rmse <= relative_rmse_thr, or if rmse
 * == 0; a converged part is FROZEN: neither its state nor its xt rows are written again, so extra steps change nothing.
 * The sums are fp64 in a fixed order that depends on the part's own row count only (no atomics): a part gives the same
 * bits alone and inside a union.  A rank-deficient covariance still yields an orthonormal R with the requested determinant.
 * state is a DEVICE double [P][GEOBI_ICP_STATE]: 0-8 R row-major, 9-11 T, 12 s, 13 rmse, 14 last relative change,
 * 15 iterations done, 16 converged (0 / 1), 17 smallest singular value of the last covariance over the largest, 18-23
 * reserved (0).
 *   geobi_icp_init    state <- init (DEVICE double [P][13]: R, T, s per part; NULL = identity), slots 13-23 = 0
 *   geobi_icp_apply   mode 0: out = s x R + T; mode 1: out = s x R^T (the linear part transposed: the gradient of mode 0
 *                     to x for a constant transform); fp64 inside, rounded once; every part, frozen or not
 *   geobi_icp_step    the step above for every part whose slot 16 is 0.  flags: bit 0 = estimate_scale (s = tr(E S) /
 *                     var(x), 1 for var(x) == 0), bit 1 = allow_reflection.  idx [Q] is clamped into the part's own rows
 *                     of y before the gather: a foreign array never reads outside y.  xt [Q, 3] is updated in place.
 *                     ws: geobi_icp_ws_bytes(xptr, P)                                                                     */
#define GEOBI_ICP_STATE 24
size_t geobi_icp_ws_bytes(const int64_t* xptr, int P);
int geobi_icp_init(void* state, int P, const double* init, void* stream);
int geobi_icp_apply(const float* x, const int64_t* xptr, int P, const void* state, int mode, float* out, void* stream);
int geobi_icp_step(const float* x, const float* y, const int32_t* idx, const int64_t* xptr, const int64_t* yptr, int P,
                   int flags, double relative_rmse_thr, void* state, float* xt, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- synthetic mesh noise ----
 * The reference has NO call site for this: its dataset is an external download (README.md:7) and the generator of its
 * noisy meshes is not in its tree.  out[v] = points[v] + displacement(v), v in [0, V); out may alias points; V == 0 is a
 * no-op.
 *   random numbers  Philox4x32-10 (Random123 constants), key = (seed & 0xffffffff, seed >> 32), counter =
 *                   (v, stream_id, draw, block): the result depends on (seed, stream_id, draw, v) only -- v is the row index
 *                   of this call -- never on grid shape, launch order or the number of calls
 *   word -> uniform u = ((w >> 9) + 0.5) * 2^-23, exact in fp32, never 0 or 1
 *   block 0         four standard normals g0..g3 by two Box-Muller pairs (words 0,1 and 2,3; cos first), precise
 *                   logf / sincosf / sqrtf
 *   direction       0 (normal): sigma * g0 * vnormal[v] (vnormal NULL is an error); 1 (random): sigma * g0 *
 *                   normalize(g1, g2, g3), (0, 0, 1) for a vector without length; vnormal is not read
 *   kind            0 (gaussian): every vertex moves; 1 (impulsive): only where u(block 1, word 0) < fraction
 * sigma >= 0 (0 leaves every bit of points alone), fraction in [0, 1]; anything else is an error.                         */
int geobi_mesh_noise(const float* points, const float* vnormal, int64_t V, float sigma, int kind, int direction,
                     float fraction, uint64_t seed, uint32_t stream_id, uint32_t draw, float* out, void* stream);

/* ---------------------------------------------------------------- surface sampling ----
 * The reference has NO call site for this: every distance of its evaluation starts from a vertex (code/data_util.py:
 * 584-616).  Points drawn uniformly by area on the surface (points [V, 3], fv [F, 3], ids in [0, V): range-check them
 * first; what is read through fv is clamped to points).  F, V >= 1; F, V, N and first + N <= GEOBI_MAX_NODES.
 *   geobi_sample_weights  integer face weights, exact from here on: d[f] = |e1 x e2| of the float32 corners widened to
 *                         fp64, every product and difference rounded on its own (no FMA contraction), non-finite -> 0;
 *                         dmax = max d, frexp(dmax) = m 2^e, exponent[0] = e (DEVICE int32, 0 for dmax == 0);
 *                         weight[f] = floor(ldexp(d[f], 32 - e)) (DEVICE int64 [F]): the largest face lands in [2^31,
 *                         2^32), a degenerate face and one below 2^-32 of the largest get 0; cum (DEVICE int64 [F]) is the
 *                         inclusive scan of weight, cum[F - 1] < 2^56.  The area is ldexp(cum[F - 1], e - 33) up to the
 *                         floors.  ws: geobi_sample_ws_bytes(F)
 *   geobi_sample_surface  sample i of the call: Philox4x32-10 with key = (seed lo, seed hi) and counter (first + i,
 *                         stream_id, draw, 2) -- blocks 0 and 1 are geobi_mesh_noise's -- gives words w0..w3;
 *                         r = w0 << 32 | w1, t = umul64hi(r, total), total = cum[F - 1] read on the device (no host sync);
 *                         out_face[i] = the first f with cum[f] > t, so a zero-weight face is never drawn; u1 = u(w2),
 *                         u2 = u(w3) with the word -> uniform map above, both replaced by 1 - u if u1 + u2 > 1;
 *                         out_bary[i] = (1 - u1 - u2, u1, u2), exact in fp32 and not negative; out_points[i] =
 *                         fma(b2, c, fma(b1, b, b0 * a)) per coordinate.  total == 0 (a mesh without area): face -1 and
 *                         zeros.  A sample depends on (seed, stream_id, draw, first + i) and the mesh only -- never on N,
 *                         the grid or how a draw is cut into calls.  N == 0 is a no-op.  Each block stages
 *                         geobi_sample_table_entries() evenly spaced entries of cum in LDS (all of cum for an F up to
 *                         that) and finishes inside the bucket from global memory: the result is the plain search's.  */
int geobi_sample_table_entries(void);
size_t geobi_sample_ws_bytes(int64_t F);
int geobi_sample_weights(const float* points, const int32_t* fv, int64_t F, int64_t V, void* weight, void* cum,
                         int32_t* exponent, void* ws, size_t ws_bytes, void* stream);
int geobi_sample_surface(const float* points, const int32_t* fv, const void* cum, int64_t F, int64_t V, int64_t N,
                         int64_t first, uint64_t seed, uint32_t stream_id, uint32_t draw, float* out_points,
                         int32_t* out_face, float* out_bary, void* stream);
/* The same for every mesh of a disjoint-union batch in one call: fv [F, 3] holds GLOBAL vertex ids into points [V, 3], the
 * HOST pointer fptr [P + 1] cuts its rows into the P meshes (fptr[0] = 0, no empty part, F = fptr[P] <= GEOBI_MAX_NODES).
 *   geobi_sample_weights_parts  every part gets its own dmax, its own exponent[p] (DEVICE int32 [P]) and its own inclusive
 *                         scan: the rows fptr[p] .. fptr[p + 1] of weight and cum (DEVICE int64 [F]) hold exactly what
 *                         geobi_sample_weights gives on mesh p alone.  cum is one scan over the union's weights (into the
 *                         workspace) minus the scan's entry before the part's first row: integer sums are exact.
 *                         ws: geobi_sample_parts_ws_bytes(F, P)
 *   geobi_sample_surface_parts  N samples per part, row p * N + i is sample i of part p: the counter is (first + i,
 *                         stream_id[p], draw, 2) with the HOST array stream_id [P], the key (seed lo, seed hi), the search
 *                         runs over the part's rows of cum.  Rows p * N .. (p + 1) * N of out_bary and out_points
 *                         ([P * N, 3]) equal, bit for bit, geobi_sample_surface on mesh p alone with stream_id[p] and the
 *                         same seed, draw and first; out_face ([P * N]) is that face plus fptr[p], a row of fv.  A part
 *                         whose total is 0: face -1 and zeros.  P * N and first + N <= GEOBI_MAX_NODES; N == 0 is a
 *                         no-op.  Workgroups are formed per part (each stages its own part's table entries in LDS), the
 *                         part table rides in the kernel arguments: more than 32 parts take several launches.            */
size_t geobi_sample_parts_ws_bytes(int64_t F, int P);
int geobi_sample_weights_parts(const float* points, const int32_t* fv, const int64_t* fptr, int P, int64_t V, void* weight,
                               void* cum, int32_t* exponent, void* ws, size_t ws_bytes, void* stream);
int geobi_sample_surface_parts(const float* points, const int32_t* fv, const void* cum, const int64_t* fptr, int P, int64_t V,
                               int64_t N, int64_t first, uint64_t seed, const uint32_t* stream_id, uint32_t draw,
                               float* out_points, int32_t* out_face, float* out_bary, void* stream);

/* ---------------------------------------------------------------- points on faces (sampled Chamfer loss) ----
 * The differentiable step from (face, barycentric) pairs, as the sampler writes them, to points and back to the vertices
 * (points [V, 3], fv [F, 3], face [n], bary [n, 3]; F, V >= 1; F, V, n <= GEOBI_MAX_NODES; ids read through fv are clamped
 * to points).  face and bary are constants of the gradient.
 *   geobi_bary_points      out[i] = fma(b2, c, fma(b1, b, b0 * a)) per coordinate, (a, b, c) = points[fv[face[i]]]: the
 *                          sampler's formula, so its out_points come back bit for bit.  face[i] outside [0, F): zeros.
 *   geobi_bary_keys        keys[3 i + k] = fv[face[i]][k] (int32 [3 n]); V for a row whose face is outside [0, F).
 *                          (segptr [V + 1], members [3 n]) = geobi_segment_csr(keys, 3 n, nseg = V): the key V is in no list.
 *   geobi_bary_points_bwd  gp[v] = sum over the entries e = 3 i + k of v's list, ascending, of bary[e] * gx[i] ([n, 3]),
 *                          products and sum in fp64, rounded once.  Every row of gp [V, 3] is written exactly once (zeros
 *                          for a vertex no sample touches); no atomics: the same bits for every run.                      */
int geobi_bary_points(const float* points, const int32_t* fv, const int32_t* face, const float* bary, int64_t V, int64_t F,
                      int64_t n, float* out, void* stream);
int geobi_bary_keys(const int32_t* fv, const int32_t* face, int64_t V, int64_t F, int64_t n, int32_t* keys, void* stream);
int geobi_bary_points_bwd(const float* bary, const float* gx, const int32_t* segptr, const int32_t* members, int64_t V,
                          int64_t n, float* gp, void* stream);

/* ---------------------------------------------------------------- bilateral normal filter ----
 * The reference has NO call site for this: its scratch code only lists result folders of classical filters beside its own
 * (code/data_util.py:732-745).  Zheng et al. 2011, local iterative scheme, over the loop-free (row, col)-sorted facet graph
 * (geobi_ring_graph_*, kind 1); the neighbourhood N(i) of face i is its row PLUS i itself.
 *   geobi_bnf_prepare    face records as 16-byte rows: rec_c [F, 4] = (centroid, area A = |cr| / 2), rec_n [F, 4] = (start
 *                        normal cr / max(|cr|, 1e-12), 0), cr = (b - a) x (c - a); fp64 inside, fp32 out.  A face of exactly
 *                        zero area gets A = 0 and the zero vector.  fv must index [0, V): range-check it first
 *   geobi_bnf_filter     n_sweeps Jacobi sweeps (ping-pong buffers, one launch per sweep: k sweeps in one call are k calls of
 *                        one sweep, bit for bit)
 *                          w_ij = A_j exp(-inv2ss |c_i - c_j|^2 - inv2sr |n_i - n_j|^2)     (differences, never expanded)
 *                          s_i = sum_{j in N(i)} w_ij n_j,  W_i = sum w_ij,  n_i' = s_i / |s_i| if |s_i| > 1e-6 W_i, else n_i
 *                        inv2ss = 1 / (2 sigma_s^2) is a DEVICE scalar (sigma_s comes from the mesh's mean centroid distance
 *                        and never visits the host; 0 for a graph without edges), inv2sr = 1 / (2 sigma_r^2).  rec_n holds
 *                        the normals to start from, out [F, 4] receives rows of rec_n's layout (so a result can be handed
 *                        back as rec_n) and must not alias a record array; n_sweeps = 0 copies rec_n.  A fixed group of 16
 *                        lanes per face with a fixed-shape reduction, no atomics: two runs give the same bits.
 *                        The spatial factor A_j exp(-inv2ss d^2), which no sweep changes, is computed once per call into
 *                        a per-edge array of the workspace.                                                             */
int geobi_bnf_prepare(const float* points, const int32_t* fv, int64_t F, int64_t V, float* rec_c, float* rec_n,
                      void* stream);
size_t geobi_bnf_filter_ws_bytes(int64_t F, int64_t E);
int geobi_bnf_filter(const float* rec_c, const float* rec_n, const int32_t* rowptr, const int32_t* col, int64_t F,
                     int64_t E, const float* inv2ss, float inv2sr, int n_sweeps, float* out, void* ws, size_t ws_bytes,
                     void* stream);

/* ---------------------------------------------------------------- guided normal filter ----
 * The reference has NO call site for this either (same list of result folders).  Zhang, Deng, Zhang, Bouaziz, Liu,
 * "Guided Mesh Normal Filtering" (Pacific Graphics 2015) over the same records, facet graph and inv2ss as the bilateral
 * filter above; the patch of face k is P_k = row k PLUS k.
 *   geobi_gnf_edge_flags     flags [E] (one byte per CSR entry): 1 when the two faces of the entry have at least 2 DISTINCT
 *                            vertex ids in common (an "edge pair": non-manifold edges, duplicate faces, faces with a
 *                            repeated vertex included), else 0.  Reads fv [F, 3] only; does not depend on the points
 *   geobi_gnf_patch_measure  H [F] from normals [F, 4] (rows of rec_n's layout):
 *                              Phi_k = max_{j, m in P_k} |n_j - n_m|;  over the edge pairs {j, m} with both faces in P_k
 *                              R_k = max |n_j - n_m| / (1e-9 + sum |n_j - n_m|), 0 without such a pair;  H_k = Phi_k R_k
 *                            16 lanes per face; the patch is staged in LDS up to 64 entries, a longer row is read through
 *                            the CSR; m in P_k is a bisection of the ascending row; the edge sum is kept in fp64; fixed-shape
 *                            reductions, no atomics: the same input gives the same bits.  H must not alias an input
 *   geobi_gnf_filter         n_sweeps Jacobi sweeps; every sweep makes H from the current normals n, then
 *                              sel_i = argmin_{k in row i or k = i} H_k, ties to the lowest face index
 *                              s = sum_{j in P_sel_i} A_j n_j,  g_i = s / |s| if |s| > 1e-6 sum A_j, else n_i
 *                              w_ij = A_j exp(-inv2ss |c_i - c_j|^2 - inv2sr |g_i - g_j|^2) over row i and j = i
 *                              s_i = sum w_ij n_j,  W_i = sum w_ij,  n_i' = s_i / |s_i| if |s_i| > 1e-6 W_i, else n_i
 *                            The edge flags (from fv) and the spatial factors are made once per call in the workspace.
 *                            sel_out: NULL, or int32 [n_sweeps, F] that receives every sweep's selection (4 B per face and
 *                            sweep).  rec_n, out, n_sweeps = 0 and the aliasing rule as geobi_bnf_filter; k sweeps in one
 *                            call are k calls of one sweep, bit for bit.
 * The patch search costs sum_k (deg_k + 1)^2 normal comparisons per sweep: a caller that admits arbitrary meshes bounds that
 * sum first (geobi_gnn_amd/filters.py does).                                                                              */
int geobi_gnf_edge_flags(const int32_t* fv, const int32_t* rowptr, const int32_t* col, int64_t F, int64_t E, uint8_t* flags,
                         void* stream);
int geobi_gnf_patch_measure(const float* rec_c, const float* normals, const int32_t* rowptr, const int32_t* col,
                            const uint8_t* flags, int64_t F, int64_t E, float* H, void* stream);
size_t geobi_gnf_filter_ws_bytes(int64_t F, int64_t E);
int geobi_gnf_filter(const float* rec_c, const float* rec_n, const int32_t* fv, const int32_t* rowptr, const int32_t* col,
                     int64_t F, int64_t E, const float* inv2ss, float inv2sr, int n_sweeps, float* out, int32_t* sel_out,
                     void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- optimiser step ----
 * torch.optim.Adam's update rule (code/train_dual.py:162, the reference's default optimiser; no amsgrad) over one flat
 * fp32 vector of n parameters, its gradient and the two moment vectors (16-byte aligned), one launch:
 *   g += weight_decay p;  m += (1 - beta1)(g - m);  v = beta2 v + (1 - beta2) g g;
 *   p -= lr / bias_corr1 * m / (sqrt(v) / sqrt(bias_corr2) + eps),      bias_corr_k = 1 - beta_k^step (host-side).  */
int geobi_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                    float weight_decay, float bias_corr1, float bias_corr2, void* stream);

/* ---------------------------------------------------------------- per-mesh rotation of a union batch ----
 * The training-time augmentation of code/dataset.py:39-69 (RandomRotate, applied per sample in `get`; the loop of
 * code/train_dual.py:141 sees every sample under its own rotation) for a batch that is already ONE disjoint-union graph:
 * rows part_ptr[p] .. part_ptr[p + 1] are turned in place by matrix p, row-vector convention as the reference's
 * `x @ R`.  One call covers one graph's arrays: the first x_triples column triples of x [n, ldx] (2 for the
 * [pos | normal] features), y [n, 3] (may be NULL) and depth_direction dd [n, 3] (may be NULL: Kinect types only); other
 * columns are not touched.  part_ptr [P + 1] (0 .. n, non-decreasing) and R [P * 9] (row-major 3x3 each) are HOST arrays
 * that travel in the kernel arguments, 32 parts per launch: no copy, no sync, stream order kept.  n == 0 is a no-op.   */
int geobi_rotate_parts(const int64_t* part_ptr, int P, const float* R, float* x, int ldx, int x_triples, float* y, float* dd,
                       int64_t n, void* stream);

/* ---------------------------------------------------------------- vertex update ----
 * data_util.update_position2 (code/data_util.py:529-556; called at code/test_dual.py:63-72 after the
 * network): n_iter Jacobi sweeps  p_v += mean_{f adj v} n_f (n_f . (c_f - p_v)), c_f = face centroid,
 * vf = padded vertex->face table [V, maxval] with -1 fill, optional projection on depth_direction.   */
size_t geobi_update_position_ws_bytes(int64_t V, int64_t F);
int geobi_update_position2(const float* points, const int32_t* fv, const int32_t* vf, int maxval,
                           const float* normals, const float* dd, int64_t V, int64_t F, int n_iter, float* out,
                           void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- mesh -> graphs ----
 * What the reference's loader computes on the CPU with openmesh / PyG before the network runs
 * (code/dataset.py:197-233 process_one_submesh).  fv = face->vertex table [F,3] int32.
 *   geobi_vertex_faces   vertex->face incidence as CSR (rowptr [V+1], list [3F], face ids ascending):
 *                        openmesh vf_indices (dataset.py:203); geobi_vf_padded emits the [V, maxval]
 *                        -1 padded table update_position2 takes; geobi_max_degree -> maxval (device int).
 *   geobi_mesh_normals   unit face normals + face centroids (dataset.py:222-224) and vertex normals =
 *                        normalised sum of incident face normals (openmesh update_vertex_normals,
 *                        dataset.py:198-199); fp64 inside, fp32 out.  vnormal may be NULL.
 *   geobi_ring_graph_*   kind 0: vertex graph = mesh edges in both directions (to_undirected(ev.T),
 *                        dataset.py:211-212); kind 1: facet graph = faces sharing >= 1 vertex
 *                        (data_util.build_facet_graph, code/data_util.py:436-456).  Output is the
 *                        (row, col)-sorted CSR WITHOUT self loops that the conv / pooling entry points
 *                        take (the reference appends / inlines one loop per node; FeaStConv and the
 *                        pooling layer drop them again).  _count writes rowptr_g [n+1] (read
 *                        rowptr_g[n] = E to size col), _fill writes col [E].
 *   geobi_calc_weight    data_util.calc_weight (code/data_util.py:383-398) over the loop-free edges:
 *                        clamp(n_i.n_j, 1e-3) * exp(|p_i-p_j|^2 / (-2 mean|p_i-p_j| + 1e-12)); the mean
 *                        runs over E + extra_zero_edges entries (the reference's edge list carries one
 *                        zero-length self loop per node).  w may be NULL; mean_len (device float,
 *                        optional) receives the mean -- center_and_scale's 1/scale (data_util.py:201-230). */
size_t geobi_vertex_faces_ws_bytes(int64_t F, int64_t V);
int geobi_vertex_faces(const int32_t* fv, int64_t F, int64_t V, int32_t* rowptr, int32_t* list, void* ws,
                       size_t ws_bytes, void* stream);
int geobi_vf_padded(const int32_t* rowptr, const int32_t* list, int64_t V, int maxval, int32_t* vf, void* stream);
int geobi_max_degree(const int32_t* rowptr, int64_t N, int32_t* out, void* stream);
int geobi_mesh_normals(const float* points, const int32_t* fv, int64_t F, int64_t V, const int32_t* rowptr,
                       const int32_t* list, float* fnormal, float* centroid, float* vnormal, void* stream);
size_t geobi_ring_graph_ws_bytes(int64_t n_nodes);
int geobi_ring_graph_count(int kind, const int32_t* fv, const int32_t* rowptr_vf, const int32_t* list,
                           int64_t n_nodes, int32_t* rowptr_g, void* ws, size_t ws_bytes, void* stream);
int geobi_ring_graph_fill(int kind, const int32_t* fv, const int32_t* rowptr_vf, const int32_t* list,
                          int64_t n_nodes, const int32_t* rowptr_g, int32_t* col, void* stream);
/* geobi_calc_weight_parts: geobi_calc_weight over a disjoint union of meshes (the patches of one network pass): node_ptr
 * [n_parts + 1] (device) cuts the nodes into parts, a part's edges are the CSR rows of its nodes, and every part gets its
 * OWN mean edge length (calc_weight normalises by the mean of the edges it is handed, code/data_util.py:383-398, and the
 * reference hands it one patch at a time) -- formed in the single-mesh kernel's order, so the weights of a part are
 * bit-identical to what the part alone gives.  The mean's denominator counts one zero-length self loop per node.        */
size_t geobi_calc_weight_parts_ws_bytes(int n_parts);
int geobi_calc_weight_parts(const float* pos, const float* normal, const int32_t* rowptr, const int32_t* row,
                            const int32_t* col, int64_t E, const int32_t* node_ptr, int n_parts, float* w, void* ws,
                            size_t ws_bytes, void* stream);
size_t geobi_calc_weight_ws_bytes(void);
int geobi_calc_weight(const float* pos, const float* normal, const int32_t* row, const int32_t* col, int64_t E,
                      int64_t extra_zero_edges, float* w, float* mean_len, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- patch split / merge ----
 * Meshes with more faces than one pass takes are cut into overlapping patches, denoised patch by patch
 * and merged (code/dataset.py:156-193, code/test_dual.py:49-61).
 *   geobi_patch_grow       data_util.mesh_get_neighbor_np (code/data_util.py:55-84) on the device: face-ring growth from
 *                          a seed until neighbor_count faces (<= 0: unlimited) or ring_count rings (<= 0: unlimited) are
 *                          listed, in the reference's visiting order (ring faces in order, their vertices in order, each
 *                          vertex's incident faces in the order of its row of `vf`, the padded [V, maxval] incidence table
 *                          of geobi_vf_padded) -- one launch of one workgroup per patch, ring by ring; a
 *                          vertex is expanded where it is first met, a face met by several expanding (face, vertex,
 *                          incidence) slots of a ring is listed where the smallest slot meets it.
 *                          `state`: geobi_patch_grow_state_ints(F, V) int32 set up by geobi_patch_grow_init (which also picks
 *                          the first seed: the face with the largest d2, lowest id on ties -- code/dataset.py:159); it
 *                          carries the visited flags from patch to patch.  seed < 0: the seed the previous call picked
 *                          (pick_next != 0: the unvisited face with the largest d2, code/dataset.py:186-190), so a CHAIN
 *                          of launches splits a mesh with no host step in between; patch_id: 1, 2, ... (distinct per
 *                          patch of one split).  sel_out: room for min(neighbor_count, F) ids; n_out (device, optional)
 *                          and mailbox (mapped host int32, optional: 1 + 2 n, written last) receive the face count; 0
 *                          faces = every face had been visited.
 *   geobi_submesh          data_util.get_submesh (code/data_util.py:318-336) on the device: sel [n_sel]
 *                          face ids -> v_idx (original vertex ids in first-use order; capacity
 *                          min(V, 3 n_sel)), f_sub [n_sel,3] renumbered faces, count (device int) = number
 *                          of patch vertices.
 *   geobi_patch_accumulate Vp[v_idx] += vert_p, sum_v[v_idx] += 1, Np[f_idx] += norm_p
 *   geobi_patch_finalize   Vp = Vp / sum_v / scale + centroid; Np = normalize(Np) (eps 1e-12)            */
size_t geobi_patch_grow_state_ints(int64_t F, int64_t V);
int geobi_patch_grow_init(int32_t* state, int64_t F, int64_t V, const float* d2, void* stream);
int geobi_patch_grow(const int32_t* fv, const int32_t* vf, int maxval, int64_t F, int64_t V, const float* d2, int64_t seed,
                     int64_t neighbor_count, int64_t ring_count, int patch_id, int32_t* state, int32_t* sel_out,
                     int32_t* n_out, int32_t* mailbox, int pick_next, void* stream);
/* n zeroed int32 slots of mapped HOST memory that a kernel can write (the patch sizes above); per host thread, valid until
 * that thread asks for more slots */
int geobi_host_mailbox(int n, int32_t** host_ptr);
/* waits (spinning) until *word != 0 and returns it; 0 when `stream` -- the one the writing kernel runs on -- drained first */
int geobi_host_mailbox_wait(const int32_t* word, void* stream);
size_t geobi_submesh_ws_bytes(int64_t n_sel, int64_t V);
int geobi_submesh(const int32_t* fv, const int32_t* sel, int64_t n_sel, int64_t V, int32_t* v_idx, int32_t* f_sub,
                  int32_t* count, void* ws, size_t ws_bytes, void* stream);
int geobi_patch_accumulate(const float* vert_p, const float* norm_p, const int32_t* v_idx, const int32_t* f_idx,
                           int64_t nv, int64_t nf, float* Vp, float* Np, int32_t* sum_v, void* stream);
int geobi_patch_finalize(float* Vp, float* Np, const int32_t* sum_v, int64_t V, int64_t F, float scale, float cx,
                         float cy, float cz, void* stream);

/* ---------------------------------------------------------------- mesh repair (weld, bad faces, compaction) ----
 * What openmesh's read_trimesh does to a file while it reads it (code/test_dual.py:30, code/dataset.py:197) and this
 * project's reader does not: a degenerate face, a second face on a directed edge ("complex edge") is refused.  Plus what
 * a triangle soup needs first: vertices with equal keys become one.  Integer-exact; nothing depends on launch geometry.
 * V, F <= GEOBI_MAX_NODES; points finite; faces index [0, V) (range-check them first: a corner outside it only makes its
 * face degenerate here, it is not reported).
 *   geobi_clean_weld     canon[v] = the LOWEST index among the vertices with v's key.  mode 0: no welding, canon[v] = v;
 *                        1: key = the three float32 bit patterns, -0.0 as +0.0; 2: key = the int32 triple
 *                        floorf(x / weld_tol) -- cells of side weld_tol, a SNAP TO A GRID and no epsilon-merge (two points
 *                        closer than weld_tol may fall into two cells), plain correctly rounded division.
 *                        counts (device int32 [2]): [0] = number of groups, [1] != 0: a quotient left the int32 range
 *                        (canon is then not to be used).  Three stable 32-bit radix passes over (key, index).
 *   geobi_clean_faces    faces_canon [F, 3] = the corners through canon; state [F]: 1 kept, 2 dropped by the half-edge
 *                        rule, 3 degenerate (two equal corners after welding); 4, "small part", is written by
 *                        geobi_topo_components only.  Half-edge rule (manifold != 0), stated
 *                        sequentially: walk the faces in ascending index; a non-degenerate face (a, b, c) is kept iff none
 *                        of a->b, b->c, c->a is owned by a kept earlier face; a kept face then owns its three.  Computed
 *                        in Jacobi rounds over the stably sorted half-edges (48-bit keys a << 24 | b): the result IS the
 *                        sequential one and *rounds (HOST int32) the same number for the same input, 0 when no face
 *                        needed a decision (manifold == 0, F == 0, degenerate faces only).  A face that shares a directed
 *                        edge with k earlier faces reads k states per round.  WAITS for `stream` (geobi_read_i32 on the
 *                        undecided counts, once per batch of rounds: 4, then 32 at a time); more than max_rounds (>= 1)
 *                        rounds is an error, never a spin.
 *   geobi_clean_compact  kept faces in their order with face_map [F'] = their input index; a vertex is used when a kept
 *                        face (state 1; every other state is dropped, 2 and 3 are counted) lists it (through canon);
 *                        used vertices in their order with their OWN coordinates
 *                        (points_out [V', 3]) and vertex_src [V'] = their input index; vertex_map [V] = new index of
 *                        canon[v] or -1.  Outputs have room for V / F rows.  counts (device int32 [5]) = V', F',
 *                        degenerate faces, faces dropped by the half-edge rule, vertices with vertex_map == -1.       */
size_t geobi_clean_weld_ws_bytes(int64_t V);
int geobi_clean_weld(const float* points, int64_t V, int mode, float weld_tol, int32_t* canon, int32_t* counts, void* ws,
                     size_t ws_bytes, void* stream);
size_t geobi_clean_faces_ws_bytes(int64_t F);
int geobi_clean_faces(const int32_t* faces, const int32_t* canon, int64_t F, int64_t V, int manifold, int max_rounds,
                      int32_t* faces_canon, int32_t* state, int32_t* rounds, void* ws, size_t ws_bytes, void* stream);
size_t geobi_clean_compact_ws_bytes(int64_t V, int64_t F);
int geobi_clean_compact(const float* points, const int32_t* faces_canon, const int32_t* state, const int32_t* canon,
                        int64_t V, int64_t F, float* points_out, int32_t* faces_out, int32_t* vertex_map,
                        int32_t* vertex_src, int32_t* face_map, int32_t* counts, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- mesh topology (winding, parts, edge report) ----
 * The stage between geobi_clean_faces and the graphs: make the winding consistent, find the connected
 * parts, report the edges.  No counterpart in the reference (openmesh refuses the faces instead).  Integer-exact; nothing
 * depends on launch geometry.  faces [F, 3] int32 are corners already taken through canon, V, F <= GEOBI_MAX_NODES; state
 * [F] may be NULL (every face 1).  A face is INCLUDED when its state is 1 and its three corners differ (and lie in [0, V));
 * the others have no links and label -1.
 *   edge table           every included face lists its undirected edges {lo, hi} (key lo << 24 | hi) in the slots 3f + k
 *                        for the corner pair (k, k + 1 mod 3); direction bit 0 when the face walks lo -> hi; opposite
 *                        corner k + 2 mod 3.  One stable 48-bit sort of (key, slot): a run lists the claimants of an edge
 *                        in ascending slot order.
 *   geobi_topo_orient    ORIENTATION LINK: a run of exactly two claimants with different opposite corners (two copies of
 *                        one triangle stay unlinked); ODD when the direction bits are equal.  label [F] = the lowest face
 *                        of the face's component over these links (-1: not included); flip [F] = the parity of odd links
 *                        on a path from that face, 0 throughout a NON-ORIENTABLE component (one with a link that
 *                        contradicts the parities); faces_out [F, 3] = the table with every flipped (a, b, c) as (a, c, b):
 *                        the lowest face of a component keeps its winding and decides for the rest.  counts (device
 *                        int32 [3]) = components, non-orientable components, flipped faces.
 *   geobi_topo_components  COMPONENT LINK: consecutive claimants of every run of two or more, whatever the direction --
 *                        faces that share an EDGE; two fans that meet in one vertex are two components.  comp [F] = the
 *                        lowest included face reachable (-1: not included); state_out [F] = the input state (1 without
 *                        one; 3 for a state-1 face with equal corners), and 4 ("small part") for every face of a component
 *                        of fewer than min_component (>= 0) faces.  counts (device int32 [3]) = components, components
 *                        below min_component, their faces.
 *   geobi_topo_report    counts (device int32 [16]) from one pass over the run heads: [0] edges, [1] boundary edges (run of
 *                        1), [2] complex edges (3 and more), [3] inconsistent edges (2 with equal direction bits); [4]
 *                        vertices an included face lists, [5] included faces, [6] the other faces; [7] components; [8]
 *                        orientation components, [9] non-orientable ones, [10] faces geobi_topo_orient would flip.
 *                        rounds: HOST int32 [2] (orientation, components).
 * The components are found in synchronous rounds over key[x] = 2 * label + parity (start 2x): a round reads `key` only and
 * lowers a copy `next` with integer atomic min -- for every link u -> w: next[parent(u)] and next[u] towards w's grandparent
 * with the parities composed, then next[x] towards x's own grandparent.  No thread reads `next` during a round and min
 * commutes: the result and *rounds (HOST int32: the rounds that changed a key, 0 without links) are functions of the input
 * alone.  A sphere of 150 k faces takes 10 rounds; WAITS for `stream` (geobi_read_i32 on the changed flags, 8 rounds at a
 * time).  More than max_rounds (>= 1) changed rounds is an error, never a spin.  One workspace size serves all three
 * (V = 0 is enough for orient and components).  F == 0 is valid.  stage_ms (HOST float [3], normally NULL) is for
 * measurement: when given, device events at the stage borders give the milliseconds of the edge table, of the rounds with
 * their waits, and of the rest, and the call waits for its own end.                                                  */
size_t geobi_topo_ws_bytes(int64_t F, int64_t V);
int geobi_topo_orient(const int32_t* faces, const int32_t* state, int64_t F, int64_t V, int max_rounds,
                      int32_t* faces_out, int32_t* flip, int32_t* label, int32_t* counts, int32_t* rounds,
                      float* stage_ms, void* ws, size_t ws_bytes, void* stream);
int geobi_topo_components(const int32_t* faces, const int32_t* state, int64_t F, int64_t V, int min_component,
                          int max_rounds, int32_t* comp, int32_t* state_out, int32_t* counts, int32_t* rounds,
                          float* stage_ms, void* ws, size_t ws_bytes, void* stream);
int geobi_topo_report(const int32_t* faces, const int32_t* state, int64_t F, int64_t V, int max_rounds, int32_t* counts,
                      int32_t* rounds, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- mesh refinement (midpoint, Loop, max-edge) ----
 * Makes a triangle mesh denser; no counterpart in the reference, whose CAD shapes were tessellated in
 * another tool.  The topology is integer-exact, positions go through ONE stated sequence of roundings (no contraction into
 * fused multiply-adds, no float atomics), nothing depends on launch geometry: tests/subdiv_model.py restates these rules
 * sequentially and reproduces every output bit.  faces [F, 3] int32 index [0, V) (range-check them first), points [V, 3]
 * float32 finite; V, F <= GEOBI_MAX_NODES.  One PASS is a plan and an emit; `loop` != 0 is the Loop scheme, `adaptive` != 0
 * the max-edge mode (midpoint positions; the two exclude each other).
 *   edge table           that of geobi_topo_*: a face is INCLUDED when its three corners differ; an included face lists
 *                        its undirected edges {lo, hi} under the key lo << 24 | hi in the slots 3f + k, edge k joining the
 *                        corners c_k and c_k+1 (indices mod 3); one stable 48-bit sort; a run of equal keys is one EDGE,
 *                        its length the claimant count n_e, its claimants in ascending slot order; edge ids count the run
 *                        heads, so they ascend with (lo, hi).  A face that is not included claims no edge and is copied
 *                        through as its single child.
 *   split edges          uniform (adaptive == 0): every edge.  Adaptive: the edges with len2 > (double)max_edge *
 *                        (double)max_edge, len2 = (dx * dx + dy * dy) + dz * dz in fp64, d = hi - lo taken in fp64 from the
 *                        float32 coordinates; strict, an edge of length exactly max_edge stays.
 *   new vertices         split edge e becomes vertex V + rank(e), rank = its position among the split edges in edge-id
 *                        order; old vertices keep the rows 0 .. V - 1.  vertex_parents [V', 2] = (v, v) for an old row,
 *                        (lo, hi) for a new one.
 *   new faces            the children of face f are consecutive rows that start at the exclusive scan of the child counts
 *                        (1 + the number of split edges of f), face_parent [F'] = f, the winding is kept; m_k = the vertex
 *                        of edge k:
 *                          0 split   (c0, c1, c2)
 *                          3 split   (c0, m0, m2) (c1, m1, m0) (c2, m2, m1) (m0, m1, m2)
 *                          1 split   (edge k; a = c_k, b = c_k+1, c = c_k+2)   (a, m_k, c) (m_k, b, c)
 *                          2 split   (edge u unsplit; a = c_u, b = c_u+1, c = c_u+2, p = m_u+1, q = m_u+2)   (p, c, q), then
 *                                    (a, b, p) (a, p, q) if edge u+1 is the longer of the two split edges, else
 *                                    (a, b, q) (b, p, q); "longer" compares the two len2, an exact tie goes to the lower
 *                                    edge id
 *                        One round conforms: a midpoint belongs to the edge, every claimant of the edge sees it.
 *   midpoint position    0.5f * lo + 0.5f * hi in float32, per coordinate (the products are exact: one rounding).
 *   Loop positions       per coordinate in fp64, rounded to float32 once at the end.  An edge is SHARP when n_e != 2; s_v =
 *                        the number of sharp edges at vertex v; the valence n = the number of edges at v.
 *                          new vertex, sharp edge       the midpoint expression above
 *                          new vertex, n_e == 2         0.375 * (lo + hi) + 0.125 * (c + d), c and d the opposite corners
 *                                                       (corner k + 2 of slot 3f + k) of its two claimants
 *                          old vertex, s_v == 0, n >= 1 beta = (n == 3) ? 3.0 / 16.0 : 3.0 / (8.0 * n); sum = the neighbours
 *                                                       added in ascending vertex id, starting from the first;
 *                                                       (1.0 - n * beta) * v + beta * sum
 *                          old vertex, s_v == 2         0.75 * v + 0.125 * (p + q), p and q the other ends of its two sharp
 *                                                       edges
 *                          old vertex otherwise         unchanged (s_v == 1, s_v >= 3, no edge)
 *                        Sharpness comes from the table of the pass itself.
 *   geobi_subdiv_plan    builds the table, the flags and the scans and leaves them in `ws`; counts (device int32 [8]): [0]
 *                        edges, [1] split edges, [2] boundary edges (n_e == 1), [3] complex edges (n_e >= 3), [4] V' = V +
 *                        split, [5] F'.  points may be NULL unless adaptive.  Nothing of the pass is written yet: the caller
 *                        reads the counts (geobi_read_i32), stops when an adaptive round splits nothing, and sizes the
 *                        outputs.  F == 0 is valid (V' = V, F' = 0, no workspace needed).  stage_ms (HOST float [3],
 *                        normally NULL) is for measurement: the milliseconds of the slots, of the sort and of the rest,
 *                        and the call then waits for its own end.
 *   geobi_subdiv_emit    over the workspace of a plan of the same faces, F, V and scheme, with the V' and F' read from its
 *                        counts (both checked against GEOBI_MAX_NODES before anything is written; a row beyond them is
 *                        never written): faces_out [F', 3], face_parent [F'], vertex_parents [V', 2], points_out [V', 3].
 *   geobi_subdiv_points  points_out [V', 3] alone, for another point array [V, 3] over the same stored plan: the same
 *                        splits, the same masks (an adaptive plan does not measure the other array).                    */
size_t geobi_subdiv_ws_bytes(int64_t F, int64_t V);
int geobi_subdiv_plan(const int32_t* faces, const float* points, int64_t F, int64_t V, int loop, int adaptive,
                      float max_edge, int32_t* counts, float* stage_ms, void* ws, size_t ws_bytes, void* stream);
int geobi_subdiv_emit(const int32_t* faces, const float* points, int64_t F, int64_t V, int loop, int64_t Vn, int64_t Fn,
                      int32_t* faces_out, int32_t* face_parent, int32_t* vertex_parents, float* points_out,
                      const void* ws, size_t ws_bytes, void* stream);
int geobi_subdiv_points(const int32_t* faces, const float* points, int64_t F, int64_t V, int loop, int64_t Vn,
                        float* points_out, const void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- mesh simplification (quadric edge collapse) ----
 * Makes a triangle mesh coarser, the inverse of geobi_subdiv_*; no counterpart in the reference.  The
 * topology is integer-exact, every float step is fp64 from the float32 inputs in ONE stated order (no contraction, no float
 * atomics; sqrt and / are the correctly rounded ones), nothing depends on launch geometry: tests/decim_model.py restates
 * these rules sequentially and reproduces every output bit.  faces [F, 3] int32 index [0, V), points [V, 3] float32 finite;
 * V, F <= GEOBI_MAX_NODES.  One ROUND is a plan and an emit and takes (points, faces) to a smaller mesh:
 *   1 edge table         that of geobi_topo_* / geobi_subdiv_*: a face is INCLUDED when its three corners differ; keys
 *                        lo << 24 | hi in the slots 3f + k, one stable 48-bit sort, a run is an EDGE, n_e its claimant count,
 *                        edge ids ascend with (lo, hi).  A face that is not included is dropped by the round and counted.
 *   2 locked vertices    a vertex with an incident edge of n_e != 2 (boundary or complex) is LOCKED: its point survives the
 *                        round with its bits unchanged (in its own row, or in the row of `lo` when it is the `hi` of a
 *                        collapsed edge).  A vertex no included face refers to keeps its row.  The NEIGHBOURS of a vertex are
 *                        the other ends of its edges (of any n_e) in ascending id, its valence their number.
 *   3 vertex quadrics    memoryless.  Included face (a, b, c), all in fp64: u = b - a, w = c - a, n = u x w (nx = uy * wz -
 *                        uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx), s = (nx * nx + ny * ny) + nz * nz.  s == 0:
 *                        the face adds nothing and takes no part in the flip test.  Else l = sqrt(s), d = -((nx * ax + ny *
 *                        ay) + nz * az), p = (nx, ny, nz, d), K_ij = (p_i * p_j) / l in the order 00 01 02 03 11 12 13 22 23
 *                        33.  Q_v starts from +0.0 and adds K entrywise over the included faces at v in ascending face id.
 *   4 candidates         an edge with n_e == 2 whose ends are not both locked.  Q = Q_lo + Q_hi entrywise.  Placements: code
 *                        0 the point of lo, 1 the point of hi, 2 0.5f * lo + 0.5f * hi in float32; with lo locked only code
 *                        0, with hi locked only code 1.  The cost of a placement (x, y, z), taken to fp64:
 *                          diag = ((Q00 * x) * x + (Q11 * y) * y) + (Q22 * z) * z
 *                          off  = ((Q01 * x) * y + (Q02 * x) * z) + (Q12 * y) * z
 *                          lin  = (Q03 * x + Q13 * y) + Q23 * z
 *                          cost = (diag + 2.0 * off) + (2.0 * lin + Q33)
 *                        The placement of least cost is taken, a tie goes to the lower code (a later code wins only with a
 *                        strictly smaller cost).  A cost that is not finite, or with use_max_cost a cost > (double)max_cost,
 *                        makes the edge no candidate.
 *   5 validity           on the round's input alone.  LINK: the neighbour lists of lo and hi share exactly two vertices.
 *                        VALENCE: both shared vertices have valence >= 4.  FLIP: every included face with s != 0 at lo or at
 *                        hi that does not hold both is recomputed with that corner at the placement (n' as n above, from the
 *                        face's own corner order); (nx * nx' + ny * ny') + nz * nz' must be > 0.
 *   6 rank               the valid candidates in ascending (cost, hash, edge id): the cost as the uint64 of its bits made
 *                        orderable (negative: all bits flipped, else the sign bit set), hash = (uint32)(((uint64)(lo << 24 |
 *                        hi) * 0x9E3779B97F4A7C15) >> 32).  The rank of a candidate is its position in that order.
 *   7 selection          GEOBI_DECIM_SWEEPS sweeps; every valid candidate starts LIVE, no vertex BLOCKED.  Per sweep: m1[v] =
 *                        the least rank of a live candidate at v; m2[v] = the least m1 over v and its neighbours; a live
 *                        candidate is SELECTED iff min(m2[lo], m2[hi]) is its own rank.  Then the ends of the sweep's
 *                        selected edges and all their neighbours are blocked, and a candidate that was selected or has a
 *                        blocked end is no longer live.  The ends of two selected edges are never in each other's closed
 *                        rings, so no face, quadric or neighbour list that one collapse changes is read by the test of another.
 *   8 budget             budget >= 0 is the face count to stop at: k = max(0, ceil((F_included - budget) / 2)) and only the
 *                        first k selected edges in rank order COLLAPSE; budget < 0: all of them.
 *   9 emit               hi merges into lo; the row of lo takes the placement.  The surviving rows keep their order
 *                        (vertex_map [V]: input row -> output row, that of lo for a merged hi); vertex_parents [V', 2] = (v, v)
 *                        or (lo, hi), place [V'] int8 = the code (0 for a row that merged nothing).  The two claimants of
 *                        every collapsed edge and the faces that are not included go, the others keep their order and
 *                        winding with their corners taken through vertex_map; face_map [F'] = the input face.
 *   geobi_decim_plan     leaves the plan in `ws`; counts (device int32 [8]): [0] edges, [1] locked vertices, [2] valid
 *                        candidates, [3] collapses, [4] V', [5] F', [6] faces not included, [7] sweeps that selected an edge.
 *                        Nothing of the round is written yet.  F == 0 is valid (V' = V, F' = 0, no workspace needed).
 *                        stage_ms (HOST float [3], normally NULL) is for measurement: the milliseconds of the tables (slots,
 *                        corner keys, three sorts), of quadrics + candidates + rank, and of selection + budget + scans; the
 *                        call then waits for its own end.
 *   geobi_decim_emit     over the workspace of a plan of the same faces, points, F, V with the V' and F' read from its
 *                        counts.  Vn, Fn are checked against what a plan of F, V can give (V - F / 2 <= Vn <= V, Fn <= F,
 *                        F - Fn >= 2 (V - Vn)) before anything is written, and no row beyond them is ever written.
 *   geobi_decim_points   out [Vn, 3]: the placements of a round replayed on another array other [V, 3] from its
 *                        vertex_parents and place alone (code 0: other[a], 1: other[b], 2: 0.5f * other[a] + 0.5f *
 *                        other[b]); parents outside [0, V) leave their row unwritten.  No workspace.                      */
#define GEOBI_DECIM_SWEEPS 3
size_t geobi_decim_ws_bytes(int64_t F, int64_t V);
int geobi_decim_plan(const int32_t* faces, const float* points, int64_t F, int64_t V, int use_max_cost, float max_cost,
                     int64_t budget, int32_t* counts, float* stage_ms, void* ws, size_t ws_bytes, void* stream);
int geobi_decim_emit(const int32_t* faces, const float* points, int64_t F, int64_t V, int64_t Vn, int64_t Fn,
                     float* points_out, int32_t* faces_out, int32_t* face_map, int32_t* vertex_map,
                     int32_t* vertex_parents, int8_t* place, const void* ws, size_t ws_bytes, void* stream);
int geobi_decim_points(const float* other, int64_t V, int64_t Vn, const int32_t* vertex_parents, const int8_t* place,
                       float* out, void* stream);

/* ---------------------------------------------------------------- isotropic remeshing (split, collapse, flip, relax) ----
 * Makes a triangle mesh REGULAR: edge lengths inside [low, high] around a target length and valences near
 * 6, by the loop of Botsch and Kobbelt; no counterpart in the reference.  The split step is geobi_subdiv_* with max_edge =
 * high; the entry points below are the other three steps and the lock flags they share.  As in 4n / 4o the topology is
 * integer-exact, every float step is fp64 from the float32 inputs in ONE stated order (no contraction, no float atomics;
 * sqrt and / are the correctly rounded ones), nothing depends on launch geometry: tests/remesh_model.py restates these rules
 * sequentially and reproduces every output bit.  faces [F, 3] int32 index [0, V), points [V, 3] float32 finite; V, F <=
 * GEOBI_MAX_NODES.  The edge table, INCLUDED faces, n_e, edge ids, NEIGHBOURS (ascending id) and valence are those of
 * geobi_decim_* (rules 1 and 2 there); the normal n of a face (p, q, r) and s = |n|^2 are those of its rule 3, from the
 * corners in the order given; (u . w) = (ux * wx + uy * wy) + uz * wz.  len2 of an edge is that of geobi_subdiv_*: d = hi -
 * lo in fp64 from the float32 coordinates, (dx * dx + dy * dy) + dz * dz.
 *   LOCK FLAGS   geobi_remesh_lock: lock [V] int32.  Bit 0: the vertex has an edge with n_e != 2 (boundary or complex).  Bit
 *                1: it has a SHARP edge.  An edge is sharp when n_e == 2 and, with n0, n1 the normals of its claimants in
 *                ascending slot order, each from its face's own row, s0 != 0 and s1 != 0 and dot = (n0 . n1) is not > 0 or
 *                dot * dot < c2 * (s0 * s1).  c2 is the fp64 cos^2 of the feature angle, formed by the caller; use_sharp = 0
 *                (a feature angle of 180 degrees) makes no edge sharp.  counts (device int32 [4]): edges, vertices with bit
 *                0, sharp edges, vertices with bit 1.
 *   SHORT-EDGE COLLAPSE   geobi_decim_plan_short: one round of geobi_decim_* with another rule 4; rules 1, 2, 5 (link,
 *                valence, flip), 6, 7, 9, the counts, geobi_decim_emit and geobi_decim_points are unchanged, there is no
 *                budget and no quadric.  A vertex is LOCKED by rule 2 or when its entry of `lock` (may be NULL) is not 0.
 *                Candidate: n_e == 2, the ends not both locked, len2 < (double)low * (double)low.  Placement: code 0 when lo
 *                is locked, else code 1 when hi is locked, else code 2.  HIGH test, before the tests of rule 5: for every
 *                neighbour w of lo and then of hi, other than lo and hi, d = w - placement in fp64; (dx * dx + dy * dy) + dz *
 *                dz > (double)high * (double)high refuses the edge.  The cost of rule 6 is len2.  0 < low <= high, finite.
 *   FLIPS        geobi_flip_plan / geobi_flip_emit, one ROUND.  The TARGET valence of a vertex is 4 with lock bit 0, else 6.
 *     candidate  an edge (a, b) = (lo, hi) with n_e == 2 whose claimants walk it in opposite directions (the direction bits
 *                of the slots differ) and which is not sharp (as above, with the use_sharp and c2 given).  c is the third
 *                corner of the face that walks lo -> hi, d that of the other; c != d.  gain = before - after, before the sum
 *                of |valence - target| over a, b, c, d, after the same with the valences of a, b one lower and of c, d one
 *                higher.  Only gain > 0 is a candidate.
 *     validity   on the round's input: the edge (c, d) does not exist; a and b have valence >= 4 (>= 3 afterwards); with
 *                n0 = n(a, b, c), n1 = n(b, a, d) the old and m0 = n(a, d, c), m1 = n(b, c, d) the new normals, (n0 . m0),
 *                (n0 . m1), (n1 . m0), (n1 . m1) and (m0 . m1) are all > 0.
 *     rank       the valid candidates in ascending (16 - gain, hash, edge id), the hash that of geobi_decim_* rule 6.
 *     selection  GEOBI_FLIP_SWEEPS sweeps of rule 7 of geobi_decim_* over the FOUR quad vertices: m1[v] = the least rank of
 *                a live candidate with v among a, b, c, d; m2[v] = the least m1 over v and its neighbours; a live candidate
 *                is SELECTED iff the least m2 of its four vertices is its own rank.  Then the four vertices of the sweep's
 *                selected candidates and all their neighbours are blocked, and a candidate that was selected or has a blocked
 *                quad vertex is no longer live.  No quad vertex of a selected flip lies in the closed ring of a quad vertex
 *                of another: two flips share no face, create different diagonals and change no valence the other counted.
 *     emit       faces_out [F, 3]: the row of the face that walked lo -> hi becomes (a, d, c), the row of the other (b, c,
 *                d); every other row is copied.  V, F, the points and the row order stay.
 *     counts     (device int32 [5]) edges, candidates (gain > 0), valid, flips, sweeps that selected.  stage_ms (HOST float
 *                [3], normally NULL): tables, candidates + rank, selection; the call then waits for its own end.
 *   RELAXATION   geobi_relax, Jacobi: reads points, writes points_out.  A vertex with a lock entry != 0 or valence < 3
 *                keeps its bits.  Else g_k = (the fp64 sum, from +0.0, of the neighbours' coordinate k in ascending id) /
 *                (double)valence; n = the componentwise fp64 sum, from +0.0, of the normals of its included faces in
 *                ascending face id, each from the face's own row; s = (n . n); s == 0: the vertex stays.  d = g - p, q = (n .
 *                d) / s, t_k = d_k - n_k * q, p'_k = (float)(p_k + lambda * t_k), lambda a double in [0, 1].  A p' equal
 *                to p in all three float32 values stays and is not counted; a p' that is not finite, or that fails the
 *                FLIP test of geobi_decim_* rule 5 over ALL included faces at the vertex with the other corners at their OLD positions, is REFUSED;
 *                every other vertex MOVES.  Then every included face with s != 0 whose normal from all three NEW positions
 *                has (n_old . n_new) not > 0 puts its moved vertices back to their old bits (REVERTED, no cascade), and the
 *                faces for which that still holds afterwards are counted (TURNED) and left.  counts (device int32 [4]):
 *                moved (before the revert), refused, reverted, turned.  stage_ms (HOST float [2]): tables, the four launches.
 *   MOVE TO      geobi_move_to: the protocol of geobi_relax with the proposal p' = target[v] (target [V, 3] float32, read
 *                as it is) in place of the tangential formula, and the same text on the device for everything else.  A
 *                vertex with a lock entry != 0 or valence < 3 keeps its bits (a vertex whose normal sum s is 0 is proposed
 *                like any other: the proposal needs no normal).  A p' equal to p in all three float32 values stays and is
 *                not counted; a p' that is not finite, or that fails the FLIP test as above, is REFUSED; every other vertex
 *                MOVES; the turned / revert / turned launches and the four counts are those of geobi_relax.  stage_ms
 *                (HOST float [2]) as there.  This is step five of the loop: the relaxed vertices go back to the input
 *                surface (target = the closest points of geobi_closest_on_faces) under the guard of the relaxation.
 *   geobi_remesh_stats   for reports: edge_len (device fp64 [3F]) = sqrt(len2) of every edge at the sorted position of its
 *                head, -1 elsewhere; valence [V].  Written for F, V > 0.
 * One workspace size serves all six entry points of this unit; F == 0 is valid everywhere (nothing flips, nothing moves:
 * geobi_relax and geobi_move_to copy the points and zero the counts). */
#define GEOBI_FLIP_SWEEPS 3
size_t geobi_remesh_ws_bytes(int64_t F, int64_t V);
int geobi_remesh_lock(const int32_t* faces, const float* points, int64_t F, int64_t V, int use_sharp, double c2,
                      int32_t* lock, int32_t* counts, void* ws, size_t ws_bytes, void* stream);
int geobi_decim_plan_short(const int32_t* faces, const float* points, const int32_t* lock, int64_t F, int64_t V, float low,
                           float high, int32_t* counts, float* stage_ms, void* ws, size_t ws_bytes, void* stream);
int geobi_flip_plan(const int32_t* faces, const float* points, const int32_t* lock, int64_t F, int64_t V, int use_sharp,
                    double c2, int32_t* counts, float* stage_ms, void* ws, size_t ws_bytes, void* stream);
int geobi_flip_emit(const int32_t* faces, int64_t F, int64_t V, int32_t* faces_out, const void* ws, size_t ws_bytes,
                    void* stream);
int geobi_relax(const int32_t* faces, const float* points, const int32_t* lock, int64_t F, int64_t V, double lambda,
                float* points_out, int32_t* counts, float* stage_ms, void* ws, size_t ws_bytes, void* stream);
int geobi_move_to(const int32_t* faces, const float* points, const float* target, const int32_t* lock, int64_t F, int64_t V,
                  float* points_out, int32_t* counts, float* stage_ms, void* ws, size_t ws_bytes, void* stream);
int geobi_remesh_stats(const int32_t* faces, const float* points, int64_t F, int64_t V, void* edge_len, int32_t* valence,
                       void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- closest points on given faces (projection) ----
 * WHERE on a surface the nearest point lies; no counterpart in the reference, whose commented-out p2m gives
 * distances only.  geobi_nearest_triangle stays the search (all pairs, fp32) and keeps its bits; this is the step after it:
 * q [Q, 3] float32, verts [V, 3] float32, fv [F, 3] int32, face [Q] int32 as geobi_nearest_triangle returned it ->
 * bary [Q, 3] float32, point [Q, 3] float32, dist [Q] float32.  One lane per query; as in 4n - 4q every float step is fp64
 * from the float32 inputs in ONE stated order (no contraction; / and sqrt are the correctly rounded ones), nothing depends
 * on launch geometry: tests/project_model.py restates these rules in plain Python and reproduces every output bit.
 *   corners      (a, b, c) = verts[fv[face[i]]] in the face row's own order, the ids clamped into [0, V) as in
 *                geobi_bary_points.  (u . w) = (ux * wx + uy * wy) + uz * wz.  p = q[i].
 *   region test  Ericson, Real-Time Collision Detection 5.1.5, in its priority order.  ab = b - a, ac = c - a, ap = p - a,
 *                bp = p - b, cp = p - c, every difference per coordinate in fp64; d1 = (ab . ap), d2 = (ac . ap), d3 = (ab .
 *                bp), d4 = (ac . bp), d5 = (ab . cp), d6 = (ac . cp): all six from ap, bp, cp directly, never from
 *                differences of d1 and d2, so a query that EQUALS a corner has three zero dot products and lands exactly
 *                in that corner's region.  vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4.  The
 *                first rule that holds decides (v, w):
 *                  1  d1 <= 0 and d2 <= 0                         corner a   (0, 0)
 *                  2  d3 >= 0 and d4 <= d3                        corner b   (1, 0)
 *                  3  vc <= 0 and d1 >= 0 and d3 <= 0             edge ab    (d1 / (d1 - d3), 0)
 *                  4  d6 >= 0 and d5 <= d6                        corner c   (0, 1)
 *                  5  vb <= 0 and d2 >= 0 and d6 <= 0             edge ac    (0, d2 / (d2 - d6))
 *                  6  va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0   edge bc    (1 - t, t), t = (d4 - d3) / ((d4 - d3) + (d5 - d6))
 *                  7  otherwise                                   inside     (vb / den, vc / den), den = (va + vb) + vc
 *                A quotient whose denominator is 0, or that is NaN, is the weight 0 (in rule 6: t = 0).  Finally v = min(max(
 *                v, 0), 1) and w = min(max(w, 0), 1 - v): a triangle without area (two or three equal corners, collinear
 *                corners) still answers with a finite point of the closed triangle -- a point OF it, not always its nearest.
 *   outputs      bary = ((float)((1 - v) - w), (float)v, (float)w).  point = the formula of geobi_bary_points on those
 *                three float32 weights, per coordinate fmaf(b2, c, fmaf(b1, b, b0 * a)) in float32: geobi_bary_points(verts,
 *                fv, face, bary) returns point bit for bit, and on another vertex array of the same V the counterpart of
 *                the projected point.  dist = (float)sqrt((ex * ex + ey * ey) + ez * ez), e_k = p_k - ((a_k + v * ab_k) + w *
 *                ac_k), in fp64 with the clamped v and w.
 *   exceptions   face[i] outside [0, F): zeros in all three outputs, as geobi_bary_points.  A query with a coordinate that
 *                is not finite: dist = +inf, bary = (1, 0, 0), point = that formula on (1, 0, 0), which is a.
 * Q, V, F >= 1 and <= GEOBI_MAX_NODES.  No workspace.                                                                      */
int geobi_closest_on_faces(const float* q, const float* verts, const int32_t* fv, const int32_t* face, int64_t Q, int64_t V,
                           int64_t F, float* bary, float* point, float* dist, void* stream);

/* ---------------------------------------------------------------- spatial grid in front of the nearest searches ----
 * A uniform grid over the box of the FINITE targets; no counterpart in the reference.  Its answer is the
 * answer of geobi_nearest_point / geobi_nearest_triangle on the same arrays BIT FOR BIT -- the same float32 distance and
 * the lowest index among equally near targets -- because a pair's squared distance comes from the same text (csrc/
 * dist_pairs.h) and the walk stops only when everything it has not visited is strictly farther than its best, by a margin
 * that covers the rounding of the binning, of the bound and of the pair function.  A target with a coordinate that is not
 * finite (a face with such a corner) is left out of box and bins: the all-pairs `<` never lets it win either.
 *   desc         HOST int32 [16], written by a plan and handed back to every later call: [0..2] cells per axis nx, ny, nz;
 *                [3..5] the box's low corner, [6..8] its high corner, [9..11] the cell edge per axis, [12] the largest
 *                target coordinate magnitude (float32 by their bits); [13] entries: the finite points, or the (cell, face)
 *                pairs; [14] the counting rounds a triangle plan took; [15] the finite targets.  Cell (x, y, z) has the id
 *                (z * ny + y) * nx + x.
 *   geobi_grid_points_plan / geobi_grid_triangles_plan   the box (two-stage min / max), then the resolution from the target
 *                count and the box alone; cells > 0 forces that many cells on every axis with extent (<=
 *                geobi_grid_max_cells()).  A triangle is filed in every cell its bounding box meets; while the entries
 *                exceed geobi_grid_entry_cap() * F the resolution is halved and counted again (one cell per axis gives at
 *                most F entries).  WAIT for `stream`: one geobi_read_i32 for the box and one per counting round, at most 9.
 *                ws: geobi_grid_plan_ws_bytes(F) (F = 0 for points).
 *   geobi_grid_points_build      cell_start [cells + 1], order [T]: the first cell_start[cells] rows of order are the
 *                finite targets sorted by (cell, index) by one stable radix sort; cell c owns order[cell_start[c] ..
 *                cell_start[c + 1]).  ws: geobi_grid_points_build_ws_bytes(T).
 *   geobi_grid_triangles_build   cell_start [cells + 1], order [desc[13]] likewise for the (cell, face) pairs, and records
 *                [F, 16] float32: the record of every face as the all-pairs walk stages it (a face without area as its
 *                longest edge), in face order; the search reads records, not corners.  ws:
 *                geobi_grid_triangles_build_ws_bytes(F).
 *   geobi_grid_nearest_point / geobi_grid_nearest_triangle   one lane per query (sorted by cell first): Chebyshev shells
 *                r = 0, 1, ... around the query's cell, at most max_rings of them (-1: geobi_grid_default_rings(); 0:
 *                none).  dist / idx (idx, face may be NULL) are written for every query that finished; the others are
 *                LEFT OVER: left [Q] holds their ids in ascending order, left_q [Q, 3] their coordinates, count (device
 *                int32 [1]) how many.  The caller reads count (geobi_read_i32), runs geobi_nearest_point /
 *                geobi_nearest_triangle on the first count rows of left_q and hands the answers to geobi_grid_scatter.
 *                The budget changes the time, never a bit.  A query that is not finite answers (+inf, 0).
 *                ws: geobi_grid_nearest_ws_bytes(Q).
 *   geobi_grid_scatter           dist[left[k]] = dist_in[k], idx[left[k]] = idx_in[k] for k < n (idx, idx_in may be NULL).
 * Q, T, V, F >= 1 and <= GEOBI_MAX_NODES; indices are int32.                                                            */
int geobi_grid_default_rings(void);
int geobi_grid_max_cells(void);
int geobi_grid_entry_cap(void);
size_t geobi_grid_plan_ws_bytes(int64_t F);
int geobi_grid_points_plan(const float* t, int64_t T, int cells, int32_t* desc, void* ws, size_t ws_bytes, void* stream);
size_t geobi_grid_points_build_ws_bytes(int64_t T);
int geobi_grid_points_build(const float* t, int64_t T, const int32_t* desc, int32_t* cell_start, int32_t* order, void* ws,
                            size_t ws_bytes, void* stream);
int geobi_grid_triangles_plan(const float* verts, const int32_t* fv, int64_t V, int64_t F, int cells, int32_t* desc, void* ws,
                              size_t ws_bytes, void* stream);
size_t geobi_grid_triangles_build_ws_bytes(int64_t F);
int geobi_grid_triangles_build(const float* verts, const int32_t* fv, int64_t V, int64_t F, const int32_t* desc,
                               int32_t* cell_start, int32_t* order, float* records, void* ws, size_t ws_bytes, void* stream);
size_t geobi_grid_nearest_ws_bytes(int64_t Q);
int geobi_grid_nearest_point(const float* q, const float* t, int64_t Q, int64_t T, const int32_t* desc, const int32_t* cell_start,
                             const int32_t* order, int max_rings, float* dist, int32_t* idx, int32_t* left, float* left_q,
                             int32_t* count, void* ws, size_t ws_bytes, void* stream);
int geobi_grid_nearest_triangle(const float* q, const float* records, int64_t Q, int64_t F, const int32_t* desc,
                                const int32_t* cell_start, const int32_t* order, int max_rings, float* dist, int32_t* face,
                                int32_t* left, float* left_q, int32_t* count, void* ws, size_t ws_bytes, void* stream);
int geobi_grid_scatter(const int32_t* left, int64_t n, int64_t Q, const float* dist_in, const int32_t* idx_in, float* dist,
                       int32_t* idx, void* stream);

/* ---------------------------------------------------------------- hole filling (boundary loops, fan fill) ----
 * Closes the holes of a triangle mesh; no counterpart in the reference.  The topology is integer-exact, a
 * new position goes through ONE stated order of fp64 additions (no float atomics), nothing depends on launch geometry:
 * tests/fill_model.py restates these rules in plain Python and reproduces every output bit.  faces [F, 3] int32 index
 * [0, V) (range-check them first), points [V, 3] float32 finite; V, F <= GEOBI_MAX_NODES.
 *   boundary slots       the edge table of geobi_topo_* / geobi_subdiv_* (the same code): a face is INCLUDED when its three
 *                        corners differ; slot s = 3f + k of an included face joins its corners k and k + 1 (mod 3); a run
 *                        of equal keys is one edge.  s is a BOUNDARY SLOT when its run has exactly one claimant.  The hole
 *                        walks it against the face: from(s) = corner k + 1, to(s) = corner k.  B = the boundary slots.
 *   simple vertices      out[v] = the boundary slots with from = v, in[v] = those with to = v.  v is SIMPLE iff out[v] ==
 *                        in[v] == 1; every other vertex with out[v] + in[v] > 0 is BLOCKED (a bow-tie where two fans meet,
 *                        a rim whose faces disagree in winding, the rim of a face next to a complex edge).
 *   successor            next(s) = the one boundary slot with from == to(s) if to(s) is simple, else none.  A simple vertex
 *                        has one incoming slot, so the slot graph is disjoint simple paths and simple cycles and nothing
 *                        runs into a cycle from outside.  s is ON A LOOP iff following next from s returns to s; otherwise
 *                        it is a CHAIN slot and is never filled.
 *   loops                the LEADER of a loop is its lowest slot; rank(s) = the steps from the leader to s; len = the slots
 *                        of the loop (3 or more by construction); the loops are numbered 0 .. L - 1 in ascending leader.
 *   selection            loop i is SELECTED iff max_hole_edges == 0 or len_i <= max_hole_edges.  The j-th selected loop, in
 *                        loop order, gets vertex V + j; its slot s gets face row F + off_j + rank(s) with the corners
 *                        (from(s), to(s), V + j), off = the exclusive scan of len over the selected loops.  The old rows
 *                        of points and faces are copied unchanged, faces that are not included and unreferenced vertices
 *                        too.  Every filled edge then has two claimants that walk it in opposite directions, and the spoke
 *                        edges are new because their far end is a new vertex: a fill never creates a complex or an
 *                        inconsistent edge.  V' = V + selected, F' = F + the sum of the selected len.
 *   position             of a new vertex, per coordinate: partial[l], l = 0 .. 63, starts at +0.0 and adds in fp64 the
 *                        coordinate of from(s) for the ranks r == l (mod 64) in ascending r; total starts at +0.0 and adds
 *                        partial[0 .. 63] in ascending l; the position is (float)(total / (double)len): one division and
 *                        one rounding.
 *   geobi_fill_plan      max_hole_edges >= 0.  Leaves the plan in `ws` and writes (each may be NULL) slot_loop [3F]: the
 *                        loop number of a slot, -1 for a slot that is no boundary slot, -2 for a chain slot; slot_rank [3F]:
 *                        rank(s), -1 off the loops; loop_leader [F] and loop_len [F]: their first L rows (L <= B / 3 <= F),
 *                        the rows beyond them are unspecified.  counts (device int32 [16]): [0] boundary edges B, [1] blocked vertices,
 *                        [2] chain edges, [3] loops L, [4] longest loop, [5] filled (selected) loops, [6] skipped loops,
 *                        [7] new faces, [8] V', [9] F'.  Nothing of the fill is written yet: the caller reads the counts
 *                        (geobi_read_i32) and sizes the outputs.  The loops come from two pointer doublings over
 *                        the B boundary slots (labels: the lowest slot reachable, a slot without successor poisons its
 *                        path; ranks: the distance to the leader), each of ceil(log2(max(3F, 2))) rounds -- a bound on
 *                        log2 B that the host knows without a read-back.  F == 0 is valid (V' = V, F' = 0, no workspace
 *                        needed).  stage_ms (HOST float [4], normally NULL) is for measurement: the milliseconds of the
 *                        edge table, of the flags / counts / successors, of the two doublings, and of the loop tables, and
 *                        the call then waits for its own end.
 *   geobi_fill_emit      over the workspace of a plan of the same faces, F, V, with the V' and F' read from its counts (both
 *                        checked against GEOBI_MAX_NODES before anything is written; a row beyond them is never written):
 *                        faces_out [F', 3], points_out [V', 3], new_vertex_loop [V' - V], new_face_loop [F' - F] (the loop
 *                        number of every new row).
 *   geobi_fill_points    points_out [V', 3] alone for another point array [V, 3] over the same stored plan: the old rows
 *                        copied, every centre taken from its own rim in that array.                                  */
size_t geobi_fill_ws_bytes(int64_t F, int64_t V);
int geobi_fill_plan(const int32_t* faces, int64_t F, int64_t V, int max_hole_edges, int32_t* slot_loop,
                    int32_t* slot_rank, int32_t* loop_leader, int32_t* loop_len, int32_t* counts, float* stage_ms,
                    void* ws, size_t ws_bytes, void* stream);
int geobi_fill_emit(const int32_t* faces, const float* points, int64_t F, int64_t V, int64_t Vn, int64_t Fn,
                    int32_t* faces_out, float* points_out, int32_t* new_vertex_loop, int32_t* new_face_loop,
                    const void* ws, size_t ws_bytes, void* stream);
int geobi_fill_points(const float* points, int64_t F, int64_t V, int64_t Vn, float* points_out, const void* ws,
                      size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- self-intersections (all pairs of faces) ----
 * Which faces of ONE mesh pass through each other; no counterpart in the reference, which never asks.  All
 * pairs, brute force: a float32 box test per pair, then an fp64 test in ONE stated order (no contraction) for the pairs
 * whose boxes overlap; nothing depends on launch geometry: tests/selfx_model.py restates these rules in numpy and
 * reproduces every output, and states the point-set definition in exact arithmetic beside them.
 * verts [V, 3] float32, faces [F, 3] int32 in [0, V) (range-check them first; an id outside makes the face degenerate),
 * state [F] int32 or NULL.  Adjacency is by INDEX: run it on a welded table (geobi_clean_weld, geobi_clean_faces).
 *   included     state == NULL or state[f] == 1, the three ids distinct, and n = (b - a) x (c - a) != (0, 0, 0).  A face
 *                that passes the state and fails one of the other two is counted as degenerate.
 *   arithmetic   every coordinate difference is the fp64 difference of two float32 values; u x w = (uy * wz - uz * wy,
 *                uz * wx - ux * wz, ux * wy - uy * wx); (u . w) = (ux * wx + uy * wy) + uz * wz; a decision is the sign of
 *                the computed value.  For integer coordinates of magnitude <= 2^14 every value is exact (differences <=
 *                2^15, products <= 2^30, cross components <= 2^31, dot products < 2^48) and so is the answer.
 *   side(T, p)   ((t1 - t0) x (t2 - t0)) . (p - t0), the corners of T in the face row's own order.
 *   axis(T)      of n = (t1 - t0) x (t2 - t0): 0, then 1 if |ny| > |nx|, then 2 if |nz| > the larger; a 2D point is the
 *                other two coordinates in ascending axis order.  o2(a, b, c) = (bu - au) * (cv - av) - (bv - av) * (cu - au).
 *   seg_tri(p, q, T)  the closed segment pq meets the closed triangle T.  dp = side(T, p), dq = side(T, q).  Both > 0 or
 *                both < 0: no.  Both == 0 (coplanar), in 2D on axis(T): yes iff o2(t0, t1, p), o2(t1, t2, p), o2(t2, t0, p)
 *                are all >= 0 or all <= 0, or pq meets one of the edges t0 t1, t1 t2, t2 t0: with o1 = o2(p, q, c), o2' =
 *                o2(p, q, d), o3 = o2(c, d, p), o4 = o2(c, d, q) for the edge cd -- all four zero: yes iff the float32
 *                boxes of pq and cd overlap (<=) in both 2D coordinates; else yes iff neither (o1, o2') nor (o3, o4) are
 *                both > 0 or both < 0.  Otherwise, with d = q - p and u_i = t_i - p: s0 = d . (u0 x u1), s1 = d . (u1 x u2),
 *                s2 = d . (u2 x u0); yes iff all >= 0 or all <= 0.
 *   pair (a, b)  a < b both included, A and B their triangles, k = the number of vertex ids they share.
 *                k = 0: no if side(A, b_i) are all > 0 or all < 0, no if side(B, a_i) are; else yes iff one of seg_tri(b0 b1,
 *                A), (b1 b2, A), (b2 b0, A), (a0 a1, B), (a1 a2, B), (a2 a0, B).  k = 1, A's corner i and B's corner j the
 *                shared one: seg_tri(a_{i+1} a_{i+2}, B) or seg_tri(b_{j+1} b_{j+2}, A), corners mod 3.  k = 2, pa and pb the
 *                corners off the shared edge uv (u, v in A's cyclic order): side(A, pb) == 0 and, in 2D on axis(A),
 *                o2(u, v, pa) and o2(u, v, pb) both > 0 or both < 0 (B folded flat onto A).  k = 3: never.
 *                The pair is always evaluated as (lower face, higher face), whichever of the two is the query.
 *   outputs      hits [F] int32: the number of faces a face intersects (0 for a face that is not included).  pairs
 *                [max_pairs, 2] int32: the pairs (a < b) in ascending (a, b) order, the first max_pairs of them; the rows
 *                beyond min(total, max_pairs) are not written; max_pairs == 0 takes pairs == NULL.  counts (device int64
 *                [8]): [0] pairs, [1] pairs with k = 0, [2] k = 1, [3] k = 2, [4] faces with hits > 0, [5] degenerate,
 *                [6] included, [7] box candidates: the pairs a < b, k < 3, whose boxes overlap (<=) -- what went to the
 *                fp64 test.  The box of a face is the exact float32 min / max of its corners.
 * F == 0 answers zeros and needs no workspace.  F, V <= GEOBI_MAX_NODES.  geobi_self_intersections_slices: the slices the
 * target faces are cut into for F faces (the rule of geobi_nearest_slices), a pure host function; every output is the same
 * for every slicing.                                                                                                      */
int geobi_self_intersections_slices(int64_t F);
size_t geobi_self_intersections_ws_bytes(int64_t F, int64_t V);
int geobi_self_intersections(const float* verts, const int32_t* faces, const int32_t* state, int64_t V, int64_t F,
                             int32_t* hits, int32_t* pairs, int64_t max_pairs, void* counts, void* ws, size_t ws_bytes,
                             void* stream);

/* ---------------------------------------------------------------- winding numbers ----
 * The generalised winding number (Jacobson et al. 2013) of query points q [Q, 3] float32 against the mesh (verts [V, 3]
 * float32, faces [F, 3] int32 range-checked by the caller): the sum of the signed solid angles of the faces seen from the
 * query, over 4 pi.  On a closed surface wound counter-clockwise seen from outside it is 1 inside and 0 outside; it needs
 * neither a closed nor a clean surface.  All pairs (csrc/winding.hip); tests/wind_model.py restates every rule in numpy.
 *   faces        a face takes part when its state is 1 (state == NULL: all), its three ids differ and lie in [0, V).
 *                With face_part [F] and query_part [Q] both given, a pair whose parts are equal is skipped.
 *   term         a, b, c = the fp64 differences of the float32 corners and the float32 query (exact), no FMA contraction:
 *                det = (ax*(by*cz - bz*cy) + ay*(bz*cx - bx*cz)) + az*(bx*cy - by*cx);  (u . w) = (ux*wx + uy*wy) + uz*wz;
 *                la = sqrt(a . a), lb, lc likewise;  den = (la*(lb*lc) + (b . c)*la) + ((a . b)*lc + (c . a)*lb);
 *                theta = 2 * atan2(det, den).  det == 0: the term is 0 (a query in the face's plane, on the face included:
 *                the principal value).  den is symmetric in b and c: a reversed face gives the negated term exactly.
 *   sum          integers: term = llrint(theta / (4 pi) * 2^40), |term| <= 2^39; the terms are added as int64 and
 *                w [Q] (DEVICE fp64) = sum * 2^-40.  The answer therefore does not depend on the slicing of the faces
 *                (geobi_winding_number_slices(Q, F): the rule of geobi_nearest_slices, a pure host function): a query gets
 *                the same bits alone and in a batch.  F <= 2^23 (|sum| <= 2^62) -- more is refused; Q, V <= GEOBI_MAX_NODES.
 * Q == 0 does nothing; F == 0 answers zeros; neither needs a workspace.
 *   geobi_part_solids  per component of geobi_topo_orient's label [F] (the lowest face of the component, -1 for a face
 *                that is not included; state as given to it), at the rows x == label[x] (the other rows: 0):
 *                volume6 [F] fp64 = the sum over the component's faces of det(v0 - o, v1 - o, v2 - o), det as above on fp64
 *                differences of float32 corners, o the first corner of face x; the faces in ascending order, face rank r
 *                into partial sum r mod 64, then the 64 partial sums added in ascending order from 0.0 (one wave, no
 *                float atomics).  closed [F] int32 = 1 iff every edge of the component has exactly two claimants;
 *                consistent [F] int32 = 1 iff no edge with exactly two claimants is walked the same way by both.
 *   geobi_flip_faces   faces_out (may be faces) = faces with corners 1 and 2 swapped where flip_of_label[label[f]] != 0
 *                (label outside [0, F): never), and flip_io[f] ^= 1 there.                                                */
int geobi_winding_number_slices(int64_t Q, int64_t F);
size_t geobi_winding_number_ws_bytes(int64_t Q, int64_t F);
int geobi_winding_number(const float* q, const float* verts, const int32_t* faces, const int32_t* state,
                         const int32_t* face_part, const int32_t* query_part, int64_t Q, int64_t V, int64_t F, void* w,
                         void* ws, size_t ws_bytes, void* stream);
size_t geobi_part_solids_ws_bytes(int64_t F);
int geobi_part_solids(const float* verts, const int32_t* faces, const int32_t* state, const int32_t* label, int64_t V,
                      int64_t F, void* volume6, int32_t* closed, int32_t* consistent, void* ws, size_t ws_bytes,
                      void* stream);
int geobi_flip_faces(const int32_t* faces, const int32_t* label, const int32_t* flip_of_label, int64_t F,
                     int32_t* faces_out, int32_t* flip_io, void* stream);

/* ---------------------------------------------------------------- dense helpers ------------
 * Plain fp32 MFMA GEMMs used by the layers above, exported for tests and profiling.            */
int geobi_gemm_nn(const float* A, int lda, const float* B, int ldb, int transB, float* C, int ldc, int M, int N,
                  int K, const float* bias, float slope, void* stream);
size_t geobi_gemm_tn_ws_bytes(int I, int J, int64_t M);
int geobi_gemm_tn(const float* A, int lda, const float* B, int ldb, int64_t M, int I, int J, float* C, int ldc,
                  void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- size read-back ------------
 * The ONE entry point that waits for the device: copies n (<= 64) int32 from device memory to `host`
 * after everything enqueued on `stream`, polling (not sleeping) until the copy has landed.  Used for the
 * data-dependent sizes of a pooling step (coarse node / edge counts; the reference's `unique` /
 * `numel() == 0` syncs, code/net_util.py:128,139).                                                  */
int geobi_read_i32(const int32_t* dev, int n, int32_t* host, void* stream);

/* ---------------------------------------------------------------- whole-network forward ----
 * The complete inference pass of code/network.py:318-343 (DualGNN.forward: vertex branch -> vertex head ->
 * geometry coupling -> facet branch -> normal head) as ONE call: the op sequence of GNNModule.forward
 * (code/network.py:270-300) and PoolingLayer.forward (code/net_util.py:76-158, edge_weight_type 10, two matching
 * steps, max or mean pooling) is driven by native host code instead of ~180 Python-level launches.  Same kernels,
 * same order, bit-identical results to the module-by-module path.
 *   arena : caller-provided device scratch; every intermediate (features, coarse graphs, cluster vectors) is
 *           bump-allocated in it and stays valid until the caller releases it.  geobi_net_forward_arena_bytes is a
 *           sufficient size for a mesh of the given level-0 sizes.
 *   graphs: loop-free, (row, col)-sorted, SYMMETRIC CSR of level 0 with the static edge weights in CSR order.
 *   out   : byte offsets into the arena of the results and of what the module surface exposes afterwards
 *           (PoolingLayer.unpooling_indices, the raw cluster vector of every matching step).
 * Host synchronisation: one read of the pooling sizes per pooling layer (4 per call).
 * Returns 0, or GEOBI_NET_FALLBACK (2) when a case outside the fast path turned up (edge-free level, a matching
 * that needs more rounds, a coarse row beyond the sort-free width) -- the caller then runs the module-by-module
 * path --, or GEOBI_NET_ARENA (3) when the arena is too small (out->used_bytes = bytes needed so far).        */
#define GEOBI_NET_FALLBACK 2
#define GEOBI_NET_ARENA 3
typedef struct { const float *lin_w, *u_w, *c, *bias; } geobi_conv_params_t;
typedef struct { geobi_conv_params_t conv[8]; } geobi_gnn_params_t;        /* l_conv1..4, r_conv1..4 */
typedef struct {
  geobi_gnn_params_t gnn_v, gnn_f;
  const float *fc_v1_w, *fc_v1_b, *fc_v2_w, *fc_v2_b, *fc_f1_w, *fc_f1_b, *fc_f2_w, *fc_f2_b;
  int32_t force_depth, pool_mean;
} geobi_net_params_t;
typedef struct {
  int64_t N, E;
  const int32_t *rowptr, *col, *row;
  const float* weight;
} geobi_level0_t;
typedef struct {
  int64_t nodes[3];               /* node count of levels 0, 1, 2 */
  int64_t unpool_off[2];          /* int32 [nodes[l]]: composed fine -> coarse index of pooling layer l + 1 */
  int64_t cluster_off[2][2];      /* int32 raw (graclus-style) cluster vector of [layer][step] */
  int64_t cluster_len[2][2];
} geobi_branch_out_t;
typedef struct {
  int64_t verts_off, normals_off, xf_off;     /* float [V,3], [F,3], [F,12] */
  int64_t used_bytes;
  geobi_branch_out_t v, f;
} geobi_net_out_t;
size_t geobi_net_forward_arena_bytes(int64_t V, int64_t Ev, int64_t F, int64_t Ef);
int geobi_net_forward(const geobi_net_params_t* prm, const geobi_level0_t* gv, const geobi_level0_t* gf,
                      const float* x_v, const float* x_f, const int32_t* fv, const float* depth_direction,
                      void* arena, size_t arena_bytes, geobi_net_out_t* out, void* stream);

/* Training through the same executor: geobi_net_forward_train additionally keeps what the backward needs in the arena
 * (size: geobi_net_train_arena_bytes) and returns a host-side record of it as *handle; geobi_net_backward replays it
 * in reverse -- the per-op backward passes of the module-by-module path, same kernels, same order -- and writes the
 * 72 parameter gradients through `grads` (same layout as the parameter struct; accumulate != 0 adds, the semantics of
 * autograd's accumulation into .grad, code/train_dual.py:211-218).  pos_rev_*: position of each level-0 edge's reverse
 * edge (geobi_csr_reverse_index).  corner_segptr / corner_members: vertex -> corner inverse lists of the face table
 * (geobi_segment_csr over fv viewed as [3F]).  The arena must stay untouched from the forward to the end of the
 * backward; geobi_net_release frees the host-side record (after the backward, or instead of it).
 * Arena: geobi_net_train_arena_bytes is an estimate from the level-0 sizes.  geobi_net_forward_train sets aside, behind
 * what it keeps, every buffer the backward will use (gradients, workspaces, the zeros that stand in for a NULL g_verts /
 * g_normals), so a successful call leaves out->used_bytes = the exact forward + backward need of this mesh, and
 * geobi_net_backward takes nothing from the arena that the forward has not set aside: it cannot run out of it.  An arena
 * too small is refused by the forward with GEOBI_NET_ARENA and no record: out->used_bytes is then the bytes needed so
 * far when the forward itself ran out, the exact total when only the backward's buffers did not fit.               */
size_t geobi_net_train_arena_bytes(int64_t V, int64_t Ev, int64_t F, int64_t Ef);
int geobi_net_forward_train(const geobi_net_params_t* prm, const geobi_level0_t* gv, const geobi_level0_t* gf,
                            const int32_t* pos_rev_v, const int32_t* pos_rev_f, const float* x_v, const float* x_f,
                            const int32_t* fv, const float* depth_direction, void* arena, size_t arena_bytes,
                            geobi_net_out_t* out, int64_t* handle, void* stream);
int geobi_net_backward(int64_t handle, const float* g_verts, const float* g_normals, const geobi_net_params_t* grads,
                       int accumulate, const int32_t* corner_segptr, const int32_t* corner_members, void* stream);
int geobi_net_release(int64_t handle);
/* Data-parallel overlap hook: the NEXT geobi_net_backward of the calling host thread records ev_main (on `stream`) and
 * ev_side (on the library's side stream, where that backward's weight-gradient products run; NULL: not wanted) at the
 * point where every gradient of gnn_f / fc_f1 / fc_f2 has been enqueued -- the facet branch's backward runs first.  A
 * caller that waits for both events on its communication stream can all-reduce that half of the gradient bucket under
 * the vertex branch's backward (hipEvent_t handles passed as void*; one-shot: cleared once recorded).              */
int geobi_net_backward_facet_events(void* ev_main, void* ev_side);
/* how often a pooling-size wait ran into its spin cap and fell back to the blocking read (diagnostic; 0 on a healthy run) */
int geobi_net_spin_cap_hits(void);

/* Several mesh groups of one optimiser step in flight together.  The reference walks the meshes of a batch one after
 * another (code/train_dual.py:199-218: forward, loss / batch_size, backward; optimiser step every batch_size meshes);
 * meshes are independent, so the iterations may overlap.  Each group (a disjoint-union graph of one or more meshes) is a
 * complete forward -> loss -> backward pipeline -- geobi_net_forward_train, the losses of code/network.py:364-396
 * (loss kinds 0 = L1, 1 = L2) and geobi_net_backward -- on its OWN stream with its OWN arena and gradient buffers, driven by
 * its own host thread inside the library (group 0 by the calling thread), so that one group's pooling chains and size
 * reads run under the other groups' FeaSt kernels.  Per-context state of the library (side streams, events, scan state)
 * is per host thread, so the groups share nothing but the read-only parameters.
 *   w_v / w_f       per-row loss weights (a union of meshes: 1 / (meshes in the group * rows of the row's mesh)); NULL: 1 / rows
 *   scale_v/scale_n factor on the group's two losses: dual_loss's v_scale / n_scale times (meshes in the group / meshes in
 *                   the step), so that the group losses ADD UP to the step's loss and the gradients to its gradient
 *   grads           where the group's 72 parameter gradients are ADDED; when they are views of one flat buffer, name it in
 *                   grad_flat / grad_count and the call zeroes it first (on the group's stream)
 *   losses          device float[2]: the group's share of loss_v and loss_n
 *   out, rc, error  filled per group (out as geobi_net_forward_train; out.used_bytes = the arena bytes this group needs)
 * Ordering: every group stream first waits for what `main_stream` holds at the call; on return `main_stream` waits for
 * every group, and, with sum_into != NULL, sum_into[i] = grad_flat_0[i] + grad_flat_1[i] + ... (fixed order: the step is
 * bit-reproducible) is enqueued on it.  The call returns when everything is ENQUEUED.  Return: 0, or the code of the first
 * failed group (GEOBI_NET_FALLBACK / GEOBI_NET_ARENA as for geobi_net_forward_train; the caller repeats the whole call). */
#define GEOBI_MAX_GROUPS 8
typedef struct {
  const geobi_level0_t *gv, *gf;
  const int32_t *pos_rev_v, *pos_rev_f;
  const float *x_v, *x_f;
  const int32_t* fv;
  const float* depth_direction;
  const float *y_v, *y_f;
  const float *w_v, *w_f;
  float scale_v, scale_n;
  const int32_t *corner_segptr, *corner_members;
  void* arena;
  size_t arena_bytes;
  geobi_net_params_t grads;
  float* grad_flat;
  int64_t grad_count;
  float* losses;
  void* stream;
  geobi_net_out_t out;
  int32_t rc;
  char error[252];
} geobi_train_group_t;
/* sizeof of a struct of this header as the library was compiled (which: 0 geobi_net_params_t, 1 geobi_level0_t,
 * 2 geobi_net_out_t, 3 geobi_train_group_t, 4 geobi_copy_seg_t; else 0): a binding checks its mirror against it */
size_t geobi_abi_sizeof(int which);
int geobi_net_train_groups(const geobi_net_params_t* prm, geobi_train_group_t* groups, int n_groups, int loss_kind_v,
                           int loss_kind_n, float* sum_into, int64_t sum_count, void* main_stream);

/* ---------------------------------------------------------------- concurrency --------------
 * Weight-gradient GEMMs are off the critical path of a backward call; by default they run on a
 * library-owned non-blocking HIP stream, forked from and joined back into `stream` INSIDE the call
 * (event wait on both ends), so the caller's stream semantics are unchanged.  0 disables it.     */
int geobi_set_overlap(int enable);
/* Deferred join (experimental, off by default): with geobi_side_defer(1) a backward call still forks the
 * side stream from `stream` but returns WITHOUT joining it.  The caller then owns the hazard: every buffer
 * handed to those calls must stay allocated and untouched until geobi_side_join(stream) has been enqueued
 * (it makes `stream` wait for everything on the side stream).                                          */
int geobi_side_defer(int on);
int geobi_side_join(void* stream);

/* ---------------------------------------------------------------- measurement --------------
 * When enabled, the selected kernel family is bracketed with HIP events on its launch stream
 * (kernel: 1 = FeaSt aggregation forward, 2 = transposed aggregation backward, 3 = backward row
 * pass, 4 = the dense GEMMs, 5 = the forms of the pooling front end: one record per scan or per geobi_match_coarsen tail,
 * tag 1 one-block scan, 2 look-back scan, 3 rocPRIM scan, 4 scan-free matching tail, 5 two-pass tail with the dual
 * one-block scan).  geobi_prof_collect synchronises the recorded events and returns the
 * launch count, the summed device time (ms) and the summed ALGORITHMIC bytes
 * of launches whose channel count equals `tag` (tag = 0: all).  For kernel 4 the third figure is the
 * flop count 2*M*N*K instead and the tag is 1 for gemm_nn (+ its split-K reduce), 2 for gemm_tn
 * (+ its slab reduce).                                                                            */
int geobi_prof_enable(int kernel);
/* diagnostic: y[i] = the kernels' own exp for the softmax (csrc/feast_dev.h: exp_le0, six instructions; arguments are
 * differences to the row maximum, i.e. FINITE and <= 0: <= 2 ulp against exp, results below 2^-126 flush to 0; a
 * non-finite argument is outside its contract).  Exposed so that a test can check it in isolation.              */
int geobi_debug_exp_le0(const float* x, float* y, int64_t n, void* stream);
/* diagnostic entries of the pooling front end (csrc/match.hip, segment.hip, pool.hip, scan.hip), for tests: forms that
 * otherwise only the executor calls.
 *   geobi_debug_scan_exclusive_i32     : the library's exclusive int scan (out[i] = in[0] + ... + in[i-1]); workspace of
 *                                        geobi_debug_scan_ws_bytes(n) bytes
 *   geobi_debug_scan_exclusive_i32_pair: two such scans of n <= 2^18 elements each in one launch (the dual scan of
 *                                        geobi_match_coarsen's two-pass tail), out_a from in_a and out_b from in_b; a
 *                                        larger n is refused.  No workspace; the pointers need no alignment beyond 4 bytes
 *   geobi_debug_segment_max2_fwd / _bwd: max over the composition of two clusterings in one pass (segptr1 / members1:
 *                                        fine -> mid lists, segptr2 / members2: mid -> coarse, every mid segment
 *                                        non-empty); arg12 [nseg2, C] = fine row of the maximum (-1: empty); the
 *                                        backward routes gout to that row (seg12 [n_fine] = composed index), add != 0:
 *                                        on top of what gx holds
 *   geobi_debug_segment_sum2           : sum over the same composition, C a multiple of 4
 *   geobi_debug_match_coarsen_rowinfo  : geobi_match_coarsen plus rowinfo [N, 4] = (r0, d0, r1, d1), start and length of
 *                                        the fine rows of each coarse node's members; rowinfo_made[0] (HOST int32) = 1 if
 *                                        the form that ran wrote it
 *   geobi_debug_pool_edge_rows_onepass : geobi_pool_edge_rows in its one-pass form (merge once, park, compact);
 *                                        E_fine = fine edge count (> 0), rowinfo_in = the array above or NULL           */
size_t geobi_debug_scan_ws_bytes(int64_t n);
int geobi_debug_scan_exclusive_i32(const int32_t* in, int32_t* out, int64_t n, void* ws, size_t ws_bytes, void* stream);
int geobi_debug_scan_exclusive_i32_pair(const int32_t* in_a, const int32_t* in_b, int32_t* out_a, int32_t* out_b, int64_t n,
                                        void* stream);
int geobi_debug_segment_max2_fwd(const float* x, int C, const int32_t* segptr1, const int32_t* members1,
                                 const int32_t* segptr2, const int32_t* members2, int64_t nseg2, float* out,
                                 int32_t* arg12, void* stream);
int geobi_debug_segment_max2_bwd(const float* gout, const int32_t* arg12, const int32_t* seg12, int C, int64_t nseg2,
                                 int64_t n_fine, float* gx, int add, void* stream);
int geobi_debug_segment_sum2(const float* x, int C, const int32_t* segptr1, const int32_t* members1,
                             const int32_t* segptr2, const int32_t* members2, int64_t nseg2, float* out, void* stream);
int geobi_debug_match_coarsen_rowinfo(const int32_t* rowptr, const int32_t* col, const float* w, int64_t N, int rounds,
                                      int init, int32_t* state, int32_t* cluster_final, int32_t* cnew, int32_t* segptr,
                                      int32_t* members, int32_t* counters, int32_t* rowinfo, int32_t* rowinfo_made,
                                      void* ws, size_t ws_bytes, void* stream);
size_t geobi_debug_pool_edge_rows_onepass_ws_bytes(int64_t nbound, int64_t E);
int geobi_debug_pool_edge_rows_onepass(const int32_t* cnew, const int32_t* segptr, const int32_t* members,
                                       const int32_t* rowptr, const int32_t* col, const float* w, const int32_t* ncount,
                                       int64_t nbound, int64_t E_fine, const int32_t* rowinfo_in, int32_t* rowptr_c,
                                       int32_t* row_c, int32_t* col_c, float* w_c, int32_t* count, int32_t* overflow,
                                       void* ws, size_t ws_bytes, void* stream);
/* diagnostic entries of the dense products (csrc/gemm.hip), for tests: forms that otherwise only the layers call, and a
 * report of the path a call took.  `plan` is a HOST array of 8 values, filled from the plan the launch itself followed.
 *   geobi_debug_gemm_nn : geobi_gemm_nn with the rest of its epilogue -- C1 / split / ldc1: columns >= split go to
 *                         C1[row * ldc1 + col - split]; ws / ws_bytes: scratch that allows split-K (automatic for few
 *                         blocks and K >= 256, or exactly fixed_slices > 1 slices; too small a scratch: one slice) --
 *                         and cfg: 0 = the launcher's own tile shape, 1..5 = the shape GEOBI_NN_CFG of that value forces
 *                         (for this call only).
 *                         plan = (FAST kernel 0/1, shape number 1..5, tile as the digits WAVES_M WAVES_N TM TN, BK, slices,
 *                         k_chunk, wide store 0/1, split-K reduce launched 0/1); all 0 when M or N is 0
 *   geobi_debug_gemm_tn : C[I, J] = sum_m A[m, I] B[m, J] with the implicit last row / column (ones_row = I - 1: a row of
 *                         ones in A^T; ones_col = J - 1: a column of ones in B; sum_row = I - 1: the column sums of B; -1:
 *                         none) and every output map: mode 0 plain (C [I, ldc]; extra_row / extra_col: the last row /
 *                         column goes to C2), 1 lin-unpack (rows (head, in-channel), C = lin.weight.grad [9 Cout, Cin],
 *                         last row -> C2 = bias.grad), 2 du/dc (A = [dp | dcs] rows 0..8 and 12..20, C = du [9, ldc],
 *                         last column -> C2 = dc [9] or NULL), 3 r' (columns [r 9 Cout | dp 12 | dcs 12]: C = lin.weight.grad
 *                         [9 Cout, Cin] at input channel col0 + row, C3 = u.weight.grad [9, Cin] or NULL; with extra_row
 *                         the last row holds column sums: C2 = bias.grad [Cout] or NULL, C4 = c.grad [9] or NULL);
 *                         accumulate != 0 adds to the outputs.  Workspace of geobi_gemm_tn_ws_bytes(I, J, M) bytes.
 *                         plan = (vector-A kernel 0/1, TI, TJ, tiles_i, tiles_j, slabs = blocks along the reduction,
 *                         rows per wave slice, bias blocks of the reduce kernel)                                          */
int geobi_debug_gemm_nn(const float* A, int lda, const float* B, int ldb, int transB, float* C, int ldc, int M, int N,
                        int K, const float* bias, float slope, float* C1, int split, int ldc1, void* ws, size_t ws_bytes,
                        int fixed_slices, int cfg, int64_t* plan, void* stream);
int geobi_debug_gemm_tn(const float* A, int lda, const float* B, int ldb, int64_t M, int I, int J, int ones_row,
                        int ones_col, int sum_row, int mode, float* C, int ldc, float* C2, float* C3, float* C4, int Cin,
                        int Cout, int col0, int extra_row, int extra_col, int accumulate, void* ws, size_t ws_bytes,
                        int64_t* plan, void* stream);
int geobi_prof_collect(int tag, int64_t* launches, double* total_ms, double* total_bytes);

#ifdef __cplusplus
}
#endif
#endif /* GEOBI_HIP_H_ */
