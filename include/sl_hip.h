/*
 * sl_hip.h - C ABI of libslhip.so, the MI355X (gfx950) engine under safe_learning_amd.
 *
 * The reference (befelix/safe_learning) has no FFI: its hot path is a Python loop that
 * feeds 10 000-cell batches to a TensorFlow graph (safe_learning/lyapunov.py:517-587,
 * safe_learning/reinforcement_learning.py:65-140, 213-279).  This header is the boundary a
 * maintainer would bind (ctypes stub in INTEGRATION.md) to replace exactly those loops; each
 * entry point cites the reference code it replaces.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes only.  Every function returns 0 (SL_OK) or a
 *    negative error code, never throws, never aborts; sl_last_error() gives the message.
 *  - "h_" pointers are host memory, copied before the call returns.  "d_" pointers are
 *    device memory owned by the caller (e.g. a torch tensor's data_ptr()) on the context's
 *    device and must stay valid until the context's stream has executed the call.
 *  - All launches go to the stream given at sl_ctx_create (a hipStream_t; NULL = the
 *    default stream) and are asynchronous unless stated otherwise.
 *  - All arithmetic is float64 (safe_learning/configuration.py:16); masks are bit masks,
 *    bit (i % 64) of word (i / 64), cell indices are flat C-order GridWorld indices
 *    (safe_learning/functions.py:622-638, 714-731).
 *  - A context is not re-entrant; use one context per GPU / per host thread.
 */
#ifndef SL_HIP_H
#define SL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libslhip.so is built with -fvisibility=hidden: only the entry points declared here are exported. */
#define SL_API __attribute__((visibility("default")))

#define SL_OK               0
#define SL_ERR_INVALID     (-1)   /* bad argument / model not set            */
#define SL_ERR_HIP         (-2)   /* a HIP runtime call failed               */
#define SL_ERR_UNSUPPORTED (-3)   /* combination not implemented             */
#define SL_ERR_NOMEM       (-4)

#define SL_MAX_STATE_DIM   6
#define SL_MAX_ACTION_DIM  2
#define SL_MAX_INPUT_DIM   8      /* state + action                          */
#define SL_MAX_GP_HEADS    6
#define SL_MAX_NN_LAYERS   4
#define SL_MAX_SIMPLICES   32     /* unit-cell simplices (Qhull gives 22 in 4-D) */

typedef struct sl_ctx sl_ctx;

/* ---- function kinds -------------------------------------------------------------- */
enum sl_policy_kind {
    SL_POLICY_LINEAR = 1,   /* u = x K^T            (LinearSystem, functions.py:1567-1583)  */
    SL_POLICY_CONST  = 2,   /* u = constant row     (reinforcement_learning.py:233-235,268) */
    SL_POLICY_TABLE  = 3,   /* u = table[i]         (per-vertex policy on the same grid)    */
    SL_POLICY_TRI    = 4,   /* u = Triangulation(x) on the auxiliary grid #1                */
    SL_POLICY_NETWORK = 5   /* u = NeuralNetwork(x)  (functions.py:1663-1729), sl_policy_network_set */
};
enum sl_dynamics_kind {
    SL_DYN_LINEAR   = 1,    /* [x,u] M^T            (functions.py:1567-1583)                */
    SL_DYN_PENDULUM = 2,    /* examples/utilities.py:242-289, 10 Euler sub-steps            */
    SL_DYN_CARTPOLE = 3,    /* examples/utilities.py:387-437, 10 Euler sub-steps            */
    SL_DYN_GP       = 4,    /* GP posterior (functions.py:417-458, 507-515, 278-291)        */
    SL_DYN_POLYNOMIAL = 5   /* term table of sl_dynamics_polynomial_set (VanDerPol: examples/utilities.py:440-519) */
};
enum sl_value_kind {
    SL_V_QUADRATIC  = 1,    /* x P x^T              (functions.py:1534-1539)                */
    SL_V_TRI        = 2,    /* Triangulation on the auxiliary grid #0 (functions.py:1473-1499) */
    SL_V_NETWORK    = 3,    /* LyapunovNetwork      (examples/utilities.py:85-104)          */
    SL_V_POLYNOMIAL = 4     /* term table of sl_value_polynomial_set (lyapunov_function_learning.ipynb cell 17) */
};
enum sl_lipschitz_kind {
    SL_LIP_CONST       = 0, /* scalar                                  (lyapunov.py:241-263) */
    SL_LIP_ABS_LINEAR  = 1, /* |x G^T| per column  (adaptive_safety_verification.ipynb c.17) */
    SL_LIP_NORM_LINEAR = 2, /* ||x G^T||_1, one column                                       */
    SL_LIP_ABS_GRAD    = 3, /* |grad V(x)| per column (inverted_pendulum.ipynb cell 14)      */
    SL_LIP_NORM_GRAD   = 4  /* ||grad V(x)||_1, one column (lyapunov_function_learning c.19) */
};

/* ---- plain-old-data model description (copied by sl_model_set) ---------------------- */
typedef struct sl_grid_desc {            /* GridWorld: functions.py:591-620 */
    int32_t d;                           /* state dimension                 */
    int32_t reserved;
    int64_t num_points[SL_MAX_STATE_DIM];
    double  offset[SL_MAX_STATE_DIM];    /* limits[:,0]                     */
    double  unit_maxes[SL_MAX_STATE_DIM];
    double  upper[SL_MAX_STATE_DIM];     /* limits[:,1]                     */
} sl_grid_desc;

typedef struct sl_policy_desc {
    int32_t kind, m, saturate, reserved;             /* Saturation: functions.py:349-354 */
    double  matrix[SL_MAX_ACTION_DIM][SL_MAX_STATE_DIM];   /* rows = outputs            */
    double  lower[SL_MAX_ACTION_DIM], upper[SL_MAX_ACTION_DIM];
    double  constant[SL_MAX_ACTION_DIM];
    const double* d_table;                           /* [nindex][m] when kind == TABLE   */
} sl_policy_desc;

typedef struct sl_dynamics_desc {
    int32_t kind, normalize;
    double  matrix[SL_MAX_STATE_DIM][SL_MAX_INPUT_DIM];    /* LINEAR: rows = outputs; GP: prior mean */
    double  tx[SL_MAX_STATE_DIM], tx_inv[SL_MAX_STATE_DIM];
    double  tu[SL_MAX_ACTION_DIM];
    double  coef[16];                    /* analytic coefficients, see sl_model.h */
} sl_dynamics_desc;

typedef struct sl_value_desc {
    int32_t kind, negate;                /* negate: V = -f (functions.py:120-122)           */
    double  matrix[SL_MAX_INPUT_DIM][SL_MAX_INPUT_DIM];    /* QUADRATIC                     */
} sl_value_desc;

enum { SL_LF_CONST = 0, SL_LF_AFFINE_NORM1 = 1 };

typedef struct sl_lipschitz_desc {
    int32_t lv_kind, lv_cols;            /* columns of L_v(x): 1 or d                       */
    double  lv_const;
    double  lv_matrix[SL_MAX_STATE_DIM][SL_MAX_STATE_DIM]; /* rows = outputs                */
    double  lf_const;                    /* L_f (closed loop): the scalar, or the constant c */
    double  tau;
    int32_t lf_kind, lf_reserved;        /* SL_LF_CONST, or SL_LF_AFFINE_NORM1:              */
    double  lf_matrix[SL_MAX_STATE_DIM][SL_MAX_STATE_DIM]; /* L_f(x) = c + ||lf_matrix x||_1  */
} sl_lipschitz_desc;                     /* (state-dependent L_f, lyapunov.py:227-244)       */

typedef struct sl_model_desc {
    sl_grid_desc      grid;
    sl_policy_desc    policy;
    sl_dynamics_desc  dynamics;
    sl_value_desc     value;             /* Lyapunov function V / value function            */
    sl_lipschitz_desc lipschitz;
    sl_value_desc     reward;            /* QUADRATIC on [x,u] (PolicyIteration only)       */
    double            gamma;             /* discount (reinforcement_learning.py:47)          */
} sl_model_desc;

/* (V, flat index) ordering key: ascending V, ties by ascending index (oracle/np_lyapunov.py). */
typedef struct sl_key { uint64_t vbits; int64_t index; } sl_key;

/* Result block of the Lyapunov passes (device memory, 8 x 8 bytes). */
typedef struct sl_sweep_result {
    sl_key   fail;          /* lexmin{(V_i,i): not (negative_i or init_i)}; vbits=~0 if none */
    sl_key   last_safe;     /* lexmax{(V_i,i) < key_star}; index=-1 if none                  */
    sl_key   max_key;       /* lexmax over all cells of the range                            */
    int64_t  count_below;   /* #cells with key < key_star                                    */
    int64_t  count_safe;    /* #bits set in the written safe mask                            */
} sl_sweep_result;

/* ---- context ------------------------------------------------------------------------- */
SL_API int  sl_version(void);
SL_API int  sl_ctx_create(int device, void* hip_stream, sl_ctx** out);
SL_API int  sl_ctx_destroy(sl_ctx* ctx);
SL_API const char* sl_last_error(const sl_ctx* ctx);      /* ctx may be NULL: last global error */
SL_API int  sl_ctx_synchronize(sl_ctx* ctx);
/* Name (with its template arguments) of the kernel(s) the last sl_lyap_sweep / sl_bellman_sweep of
 * this context launched for the per-cell work, e.g. "k_gp_sweep4<d=4, m=1, xs_global=0>" or
 * "k_gp_sweep<...> + k_nn_check_mfma<...>" for a two-pass sweep; "" before the first sweep.  The
 * string lives in the context and is overwritten by the next sweep. */
SL_API const char* sl_last_kernel(const sl_ctx* ctx);
/* Kernel durations for benchmarks.  With slots > 0 every sl_lyap_sweep (channel 0),
 * sl_lyap_finalize_dev (channel 1) and sl_bellman_sweep (channel 2) brackets its launches with a pair
 * of HIP events on the context's stream, up to `slots` calls per channel (later calls are not
 * recorded); the events are created here, not per call.  slots = 0 switches it off and frees them.
 * sl_timing_collect waits for the recorded calls of one channel, writes their durations in
 * milliseconds to h_ms (at most `capacity`), the number written to *count, and empties the channel.
 * (The reference has no counterpart: its timings are the notebooks' wall clocks.) */
SL_API int  sl_timing_configure(sl_ctx* ctx, int slots);
SL_API int  sl_timing_collect(sl_ctx* ctx, int channel, double* h_ms, int capacity, int* count);

/* ---- model upload (copies; replaces the TF graph build of lyapunov.py:431-443) --------- */
SL_API int  sl_model_set(sl_ctx* ctx, const sl_model_desc* h_model);
/* A policy table (SL_POLICY_TABLE: policy.d_table, or the slot-1 table of SL_POLICY_TRI) was
 * overwritten IN PLACE.  What the sweeps derive from the policy alone - k_bellman4_policy's distinct
 * actions and tile order, the select arrays of the successor cache - is kept between calls until the
 * policy changes, and sl_model_set sees a change only in the description's bytes: the same pointer
 * with new values is the same description.  Call this after such an edit (before the next sweep);
 * handing in another pointer (sl_model_set, sl_tri_set_table) needs no call. */
SL_API int  sl_policy_touch(sl_ctx* ctx);

/* Polynomial dynamics (SL_DYN_POLYNOMIAL): a vector field given as data, nterms terms
 *     coef * prod_q z_q^e_q,   z = [x, u] (d + m entries),
 * term t adding to output row h_rows[t] in [0, d).  h_exponents is [nterms][SL_MAX_INPUT_DIM] (entries at
 * q >= d + m must be 0); the sum of a term's exponents is at most SL_POLY_MAX_DEGREE, nterms at most
 * SL_POLY_MAX_TERMS (0: the zero field); a row may have no term.  The table is copied (sorted by row, the
 * caller's order kept within a row).  One call x -> x+ of the dynamics (csrc/sl_polynomial.h states the
 * operation order, multiplications and additions only, powers by repeated multiplication):
 *     substeps > 0:  `substeps` explicit-Euler steps z_i <- z_i + h * p_i(z), all rows from the same z,
 *                    the action entries held (h = dt / substeps is the caller's);
 *     substeps = 0:  the polynomial is the map itself, x+_i = p_i(z) (h is not used).
 * sl_dynamics_desc's normalize / tx / tx_inv / tu apply as for the pendulum: z = [x * tx, u * tu] going in,
 * x+ * tx_inv coming out; its other fields are not read.  sl_model_set accepts kind SL_DYN_POLYNOMIAL only
 * when the table's d and m are the model's.  A new table is a new model: everything the context derived
 * from the dynamics (successor cache, policy-select arrays) is dropped.  Action tangents are not implemented:
 * sl_critic_batch, sl_action_gradient and sl_decrease_gradient return SL_ERR_UNSUPPORTED for this kind. */
#define SL_POLY_MAX_TERMS  64
#define SL_POLY_MAX_DEGREE 8      /* total degree of one term: at most 8 multiplications per term */
SL_API int  sl_dynamics_polynomial_set(sl_ctx* ctx, int d, int m, int nterms, const int32_t* h_rows,
                    const double* h_coef, const uint8_t* h_exponents, int substeps, double h);

/* Polynomial Lyapunov / value function (SL_V_POLYNOMIAL): a candidate given as data, nterms terms
 *     V(x) = sum_t coef_t * prod_q z_q^e_tq,   z_q = x_q * h_tx[q] (normalize != 0) or x_q,
 * h_exponents is [nterms][SL_MAX_STATE_DIM] (entries at q >= d must be 0); the sum of a term's exponents is at
 * most SL_POLY_MAX_DEGREE.  The call validates, builds the device table - the value row and one row per
 * partial derivative (every term with e_k >= 1 gives coef * e_k and the exponents with e_k - 1) - waits for the
 * stream and uploads; value row and gradient rows together hold at most SL_POLYV_MAX_ENTRIES entries (a full
 * quartic in four states: 69 + 4 * 35; a full sextic in three: 83 + 3 * 56).  csrc/sl_poly_value.h states the
 * operation order: multiplications and additions only, powers by repeated multiplication, the gradient with
 * respect to x (times h_tx[k]).  sl_value_desc.negate applies; its matrix is not read.  sl_model_set accepts
 * kind SL_V_POLYNOMIAL only after this call and only when the table's d is the grid's.  SL_LIP_ABS_GRAD and
 * SL_LIP_NORM_GRAD take the table's gradient.  A new table is a new value function; a table of another d than
 * that of a set model of the kind unsets the model (the entry points then ask for sl_model_set again).  The sweeps, sl_values and
 * sl_eval_points (also SL_EVAL_GRADIENT) take the kind; second derivatives are not implemented:
 * sl_decrease_gradient returns SL_ERR_UNSUPPORTED for it, and the Bellman entry points take tables only. */
#define SL_POLYV_MAX_ENTRIES 256
SL_API int  sl_value_polynomial_set(sl_ctx* ctx, int d, int nterms, const double* h_coef,
                    const uint8_t* h_exponents, int normalize, const double* h_tx);

/* GP head `head` of the dynamics (FunctionStack: one head per output column,
 * functions.py:278-291; a shared-kernel multi-output GPRCached is one head with dout = D).
 *   h_X      [n][p]   training inputs                     (GPRCached.X,      functions.py:382)
 *   h_Linv   [n][n]   inverse of the Cholesky factor of K + sigma_n^2 I, lower triangular,
 *                     so that a = Linv k_x equals tf.matrix_triangular_solve (functions.py:441)
 *   h_alpha  [n][dout] L^-1 (Y - m(X))                    (GPRCached.alpha,  functions.py:405-409)
 * RBF (gpflow 0.4.0): k = variance * exp(-0.5 sum_q ((x_q - x'_q) / lengthscales_q)^2). */
SL_API int  sl_gp_set_head(sl_ctx* ctx, int head, int n, int p, int dout, int col0,
                    const double* h_X, const double* h_Linv, const double* h_alpha,
                    double variance, const double* h_lengthscales);
/* The same head with a kernel of the family the reference's notebooks build from gpflow 0.4.0's
 * kernels.py (examples/inverted_pendulum.ipynb:152-158: Linear + Matern32 * Linear; the functions
 * GPRCached calls are kern.K and kern.Kdiag, functions.py:401, 438, 445, 450): a SUM of PRODUCTS
 * of leaf kernels.  Factor f belongs to product `product` (products are numbered 0, 1, ... in
 * the order of their first factor; the factors of a product are adjacent):
 *   SL_KERNEL_RBF       variance[0] exp(-r2 / 2),                    r2 = sum_q ((x_q - x'_q) inv_lengthscales[q])^2
 *   SL_KERNEL_MATERN32  variance[0] (1 + sqrt(3) r) exp(-sqrt(3) r), r = sqrt(r2 + 1e-12)   (Stationary.euclid_dist)
 *   SL_KERNEL_LINEAR    sum_q variance[q] x_q x'_q
 * Dimensions outside a leaf's active_dims carry inv_lengthscales[q] = 0 (variance[q] = 0 for a
 * Linear leaf).  K(x, x) of the posterior variance (functions.py:450) follows from the same
 * formulas (Kdiag).  The inputs are stored unscaled. */
#define SL_KERNEL_RBF 0
#define SL_KERNEL_MATERN32 1
#define SL_KERNEL_LINEAR 2
#define SL_KERNEL_MAX_FACTORS 8
typedef struct sl_gp_kernel_factor {
    int32_t kind, product;
    double  variance[SL_MAX_INPUT_DIM];
    double  inv_lengthscales[SL_MAX_INPUT_DIM];
} sl_gp_kernel_factor;
typedef struct sl_gp_kernel {
    int32_t nfactors, reserved;
    sl_gp_kernel_factor factor[SL_KERNEL_MAX_FACTORS];
} sl_gp_kernel;
SL_API int  sl_gp_set_head_kernel(sl_ctx* ctx, int head, int n, int p, int dout, int col0,
                    const double* h_X, const double* h_Linv, const double* h_alpha,
                    const sl_gp_kernel* h_kernel);
/* One more training point for an uploaded head (GaussianProcess.add_data_point,
 * functions.py:525-546) without re-packing: the rank-one extension of the cached factors touches
 * one new row of L^-1, so only that row is scattered into the fragment layout.
 *   h_x [p], h_linv_row [n+1] = row n of the extended L^-1 (lower triangle incl. the diagonal),
 *   h_alpha_new [dout] = the new last row of alpha = L^-1 (Y - m(X)).
 * alpha' = Linv^T alpha gets the rank-one term linv_row * alpha_new.  Returns SL_ERR_UNSUPPORTED
 * when the padded capacity of the head is exhausted (then call sl_gp_set_head again). */
SL_API int  sl_gp_append_point(sl_ctx* ctx, int head, const double* h_x, const double* h_linv_row,
                        const double* h_alpha_new);
/* The variance floor of k_gp_sweep4's early decision in use for `head`, read back from the device words
 * the kernel reads: out[s], s = 0 .. n - 1 (n at most 32), is the constant c_s with  posterior variance of
 * all points >= c_s x posterior variance of the first 256 s points,  which lets the lower bound of the
 * decrease use err = beta sqrt(c_s var) instead of err = 0.  sl_gp_set_head certifies the constants on the
 * host from h_Linv - O(n^3), 1.2 s at 1024 points - for the heads that can use them: RBF, more than 192 and
 * at most 2048 points, in a context whose early decision is on (sl_gp4_early_configure) and whose
 * configuration is not forced when the head is uploaded.  0 = no floor: every other head, boundaries at
 * or behind the last point, any doubt.  sl_gp_append_point sets them all to 0 until the next
 * sl_gp_set_head. */
SL_API int  sl_gp_variance_floor(sl_ctx* ctx, int head, double* out, int n);
SL_API int  sl_gp_configure(sl_ctx* ctx, int nheads, double beta);
/* k_gp_sweep4 (one shared-kernel RBF head of more than 256 points, closed-form policy, quadratic V,
 * no record output) computes the posterior mean of a 64-cell tile first and stops adding variance
 * panels once bounds of the decrease - err = beta sqrt(variance floor) from below (sl_gp_variance_floor;
 * err = 0 without one), err = beta sqrt(variance - partial |a|^2) from above - settle the mask bit of every cell: the same bits, fewer flops.  enable = 0 runs every
 * panel of every tile (the A/B baseline and the other side of the bit-identity tests); the default
 * is 1.  Takes effect at the next sweep. */
SL_API int  sl_gp4_early_configure(sl_ctx* ctx, int enable);
/* At most `workgroups` workgroups per launch of k_gp_sweep4 (0, the default: as many as the device
 * holds).  For tests: on a small grid one workgroup then draws many tiles, and the queues of its open
 * 16-cell blocks fill composite tiles from different source tiles.  The value belongs to the
 * context and takes effect at its next sweep. */
SL_API int  sl_gp4_workgroups_configure(sl_ctx* ctx, int workgroups);
/* A block-mode launch of k_gp_sweep4 that is large enough for the tile counter decides the blocks in
 * a kernel of its own (k_gp_mean_blocks), segment by segment of source tiles, and runs the panels on
 * the list of open blocks each segment leaves.  tiles > 0: every block-mode launch does, in segments
 * of `tiles` source tiles (tests: several segments, empty and ragged lists on small grids); 0, the
 * default: large launches only, the segment size from the scratch budget.  Belongs to the context,
 * takes effect at its next sweep. */
SL_API int  sl_gp4_segment_configure(sl_ctx* ctx, int tiles);
/* Block mode of k_gp_sweep4 decides and queues 8-cell HALVES of the 16-cell blocks: a half the
 * bounds decide leaves at once, and the variance panels run on slots that hold one whole block or the
 * low half of one block beside the high half of another.  enable = 0 goes back to whole blocks (A/B
 * runs and tests; the results are the same bits either way).  sl_last_kernel reports, per launch, the
 * paired composites and the slots of them that held one half only.  Belongs to the context, takes
 * effect at its next sweep. */
SL_API int  sl_gp4_halves_configure(sl_ctx* ctx, int enable);
/* A segmented block-mode sweep first decides, in a streaming pass (k_gp_mean_lattice, k_gp_predecide),
 * the 16-cell blocks that a bound of the posterior mean shows to fail whatever their variance: the
 * first-order Taylor expansion of the mean about a reference cell with the remainder
 * |g_j(z) - g_j(z_c) - J_j (z - z_c)| <= (sqrt(3) / 2) ||g_j||_H s |z - z_c|^2, the reference cells on a lattice
 * of every `spacing`-th grid index per axis (and the last index of the axis).  Closed-form policies only.  k_gp_mean_blocks skips those
 * blocks.  The results are the same bits either way; sl_last_kernel reports the blocks decided.
 * enable = 0 switches the pass off (A/B runs and tests); spacing = 0 keeps the spacing (default 8).
 * Belongs to the context, takes effect at its next sweep. */
SL_API int  sl_gp4_predecide_configure(sl_ctx* ctx, int enable, int spacing);
/* The blocks that pass left open, as the list the mean pass of the context's LAST sweep worked through:
 * 32-bit block numbers 4 tile + jb in ascending order (tile t of the shard starts at cell lo + 64 t,
 * block jb 16 jb cells further).  *count = the list's length; the first min(cap, *count) entries
 * go to out (cap = 0: the length only); *used = 1 when the mean pass ran from the list
 * (k_gp_mean_open), 0 when the sweep had none - no deciding pass, or a shard of 2^29 tiles or more -
 * and then *count = 0.  Waits for the context's stream.  For tests and diagnostics. */
SL_API int  sl_gp4_open_list(sl_ctx* ctx, uint32_t* out, int64_t cap, unsigned long long* count, int* used);

/* Auxiliary grid #slot with a per-vertex table (Triangulation: functions.py:1002-1032,
 * 1064-1101): slot 0 = value function, slot 1 = policy.  h_simplices [nsimplex][d+1] are the
 * unit-cell vertices as {0,1}^d corner codes (bit k = dimension k), h_hyperplanes
 * [nsimplex][d][d] = inv(vertices[1:] - vertices[0]); d_table [nindex][ncols] stays caller-owned. */
SL_API int  sl_tri_set(sl_ctx* ctx, int slot, const sl_grid_desc* h_grid, int nsimplex,
                const int32_t* h_simplices, const double* h_hyperplanes,
                const double* h_discrete_points, int project, int ncols, const double* d_table);
/* New vertex values for a slot whose grid stays.  Call it (or sl_policy_touch) whenever the values of
 * the POLICY table (slot 1) change, also when they were overwritten in place: what the
 * policy-evaluation sweep derives from the policy alone is kept between sweeps until this,
 * sl_policy_touch, sl_tri_set(slot 1) or an sl_model_set with another policy description says that
 * the policy is a new one. */
SL_API int  sl_tri_set_table(sl_ctx* ctx, int slot, const double* d_table);

/* LyapunovNetwork (examples/utilities.py:85-104): h_kernels = per-layer kernel matrices
 * [out_i][in_i] concatenated; activation codes 0 = linear, 1 = tanh, 2 = relu. */
SL_API int  sl_network_set(sl_ctx* ctx, int nlayers, const int32_t* h_dims /* nlayers+1 */,
                    const int32_t* h_activations, const double* h_kernels);

/* NeuralNetwork as the policy (functions.py:1663-1729; the policies of examples/inverted_pendulum.ipynb
 * :215 and of the reinforcement-learning notebooks): a chain of dense layers
 *   net <- act_l(net W_l + b_l),  u = output_scale * net
 * h_dims [nlayers + 1] = input width (the state dimension) followed by the units of every layer (the
 * reference's `layers`), widths <= 64, the last <= SL_MAX_ACTION_DIM; h_activations [nlayers]: 0 none,
 * 1 tanh, 2 relu, 3 sigmoid; h_kernels = the W_l ([in][out] row-major, tf.layers.dense's kernel)
 * concatenated; h_has_bias [nlayers] (may be NULL: none) and h_biases = the b_l of the layers that
 * have one, concatenated (the reference's output layer never has).  With policy.kind =
 * SL_POLICY_NETWORK the entry points that evaluate the policy (sl_lyap_sweep, sl_bellman_sweep with
 * n_actions == 0, sl_eval_points) evaluate the network once per cell / vertex / point into an
 * action table of their own and run the kernels on that table (policy.saturate applies as usual). */
SL_API int  sl_policy_network_set(sl_ctx* ctx, int nlayers, const int32_t* h_dims,
                           const int32_t* h_activations, const double* h_kernels,
                           const double* h_biases, const int32_t* h_has_bias, double output_scale);

/* ---- Lyapunov passes ------------------------------------------------------------------- */
/* values[i-lo] = V(all_points[i]), i in [lo,hi): the points of functions.py:622-638 (np.linspace:
 * the last point of each dimension is exactly the upper limit).  Replaces
 * Lyapunov.update_values (lyapunov.py:305-322). */
SL_API int  sl_values(sl_ctx* ctx, int64_t lo, int64_t hi, double* d_values);

/* Decrease check of every cell i in [lo,hi) (lo % 64 == 0): policy -> dynamics ->
 * V(f(x)) - V(x) + L_v.err < -|L_v|_1 (1 + L_f) tau  (lyapunov.py:436-441, 265-288, 324-376).
 * Replaces the batch loop lyapunov.py:524-587.
 *   d_init_bits   in  (may be NULL) cells that count as safe without a check
 *   d_values      in  V on the grid from sl_values: the ordering keys of lyapunov.py:512
 *                     (may be NULL: the V(x_i) computed for the decrease is used instead)
 *   d_neg_bits    out the `negative` mask
 *   d_result      out ->fail = lexmin over failing cells (other fields untouched)
 *   d_dbg         out (may be NULL) per cell [decrease, threshold, mean[d], err[d]] */
SL_API int  sl_lyap_sweep(sl_ctx* ctx, int64_t lo, int64_t hi, const uint64_t* d_init_bits,
                   const double* d_values, uint64_t* d_neg_bits, sl_sweep_result* d_result,
                   double* d_dbg);

/* ---- the level set: every decision is read from DEVICE memory (no host round trip between the
 * passes of one update_safe_set; the multi-GPU path of SURVEY.md 8e) ------------------------------ */

/* *out = 1 when d_values may be NULL in sl_lyap_sweep AND in the three passes below: V is a
 * QuadraticFunction (functions.py:1503-1539) on a grid of 1..4 dimensions (last axis a multiple of 8
 * cells) whose np.linspace points
 * (functions.py:612-638, the points Lyapunov.update_values evaluates V on, lyapunov.py:321) equal
 * index_to_state (functions.py:728-731) bit for bit.  The ordering keys of lyapunov.py:512 are then
 * recomputed from the cell index (8 cells of a grid row per thread, the prefix of the ordered sums
 * shared) instead of read: the values array (2.1 GB at 128^4) need not exist. */
SL_API int  sl_values_implicit(sl_ctx* ctx, int* out);

/* d_out = fold of `count` result records that lie in device memory (e.g. every rank's record after
 * an all-gather): lexmin of `fail`, lexmax of `last_safe` and `max_key`, sums of the counters -
 * the reductions np.argsort + the batch loop of lyapunov.py:512-595 perform on one host. */
SL_API int  sl_fold_results(sl_ctx* ctx, const sl_sweep_result* d_records, int count,
                     sl_sweep_result* d_out);

/* safe_i = init_i | (key_i < key_star) | (prev_i & key_i >= key_keep), the parallel form of
 * lyapunov.py:513-606, with key_star = d_folded->fail and key_keep = *d_keep (NULL:
 * none) read by the kernel.  d_init_bits and d_prev_bits may be NULL, d_values too
 * (sl_values_implicit).  d_result: ->fail is copied from d_folded; last_safe, max_key, count_below
 * and count_safe are this range's statistics (fold them across ranks with sl_fold_results). */
SL_API int  sl_lyap_finalize_dev(sl_ctx* ctx, int64_t lo, int64_t hi, const double* d_values,
                          const uint64_t* d_init_bits, const uint64_t* d_prev_bits,
                          const sl_sweep_result* d_folded, const sl_key* d_keep,
                          uint64_t* d_safe_bits, sl_sweep_result* d_result);

/* The refinement array N(x) of lyapunov.py:220-225 through a NON-adaptive update with
 * can_shrink = False (lyapunov.py:507-510, 531, 585-587, 601-606), in place on this range's cells:
 *   ref_i <- init_i ? 1 : key_i < key* ? (negative_i ? 1 : ref_i) : (key_i >= key_keep ? ref_i : 0)
 * with key* = d_folded->fail, key_keep = *d_keep (NULL: no failure, nothing is cleared), d_neg_bits the
 * sweep's `negative` words.  Only needed when an adaptive update left values other than 0 / 1. */
SL_API int  sl_refinement_carry(sl_ctx* ctx, int64_t lo, int64_t hi, const double* d_values,
                         const uint64_t* d_init_bits, const uint64_t* d_neg_bits,
                         const sl_sweep_result* d_folded, const sl_key* d_keep, int64_t* d_refinement);

/* Radix select of the k-th smallest (V, index) key over all ranks (0-based; what
 * values[order[k]] of lyapunov.py:512, 590-595 reads) with its state in device memory. */
typedef struct sl_select_state {
    uint64_t prefix;        /* digits found so far (of vbits, then of the index)                 */
    int64_t  remaining;     /* rank among the keys that share the prefix                         */
    sl_key   key;           /* the result once both phases are through; KEY_NONE if none         */
    int64_t  rank;          /* the k the select was started with                                 */
    int64_t  none;          /* 1: k >= n_total (no such key), every pass is a no-op              */
    int64_t  pad[2];
} sl_select_state;          /* 64 bytes */

/* k >= 0: select that rank.  k < 0: rank = (d_folded->count_below / batch + 1) * batch, the first
 * position behind the batch that holds the first failure (lyapunov.py:585-587: later batches keep
 * their previous state).  n_total = cells of the whole grid. */
SL_API int  sl_select_begin(sl_ctx* ctx, sl_select_state* d_state, int64_t k, int64_t batch,
                     const sl_sweep_result* d_folded, int64_t n_total);
/* One radix-select pass over the (V, index) keys of [lo,hi): the 256-bin histogram of byte `byte`
 * (7 = most significant, taken first) of the vbits (which = 0) or of the index (which = 1, only cells
 * with vbits == state->key.vbits), among the keys whose higher bytes equal the state's prefix.
 * d_values may be NULL (sl_values_implicit).  d_hist[256] is zeroed and filled, not added to: SUM it
 * over the ranks, then call sl_select_digit, which takes the digit that holds the rank into the
 * prefix.  Eight passes of which = 0, then eight of which = 1, give the k-th order statistic that
 * lyapunov.py:590-595 reads through argsort. */
SL_API int  sl_select_hist(sl_ctx* ctx, int64_t lo, int64_t hi, const double* d_values, int which,
                    int byte, const sl_select_state* d_state, uint64_t* d_hist);
SL_API int  sl_select_digit(sl_ctx* ctx, int which, int byte, const uint64_t* d_hist,
                     sl_select_state* d_state);

/* ---- the adaptive branch of update_safe_set (lyapunov.py:445-487, 540-582) -------------------------
 * The reference walks the cells in ascending-V order in batches of config.gp_batch_size; a batch whose
 * unsafe tail can be accepted through local refinement lets the loop go on, the first one that
 * cannot ends it.  Every batch is judged on its own from per-cell rows in sorted order. */

/* Stable ascending sort of n (key, value) pairs by key: eight 8-bit radix passes (np.argsort of
 * lyapunov.py:512 with ties in input order).  Result in d_keys / d_vals; d_keys_tmp / d_vals_tmp [n]
 * and d_counts [SL_SORT_COUNT_WORDS] are scratch. */
#define SL_SORT_COUNT_WORDS (256 * 2048)
SL_API int  sl_sort_pairs(sl_ctx* ctx, int64_t n, uint64_t* d_keys, int64_t* d_vals,
                   uint64_t* d_keys_tmp, int64_t* d_vals_tmp, uint32_t* d_counts);
/* Stable partition: d_perm = the positions 0..n-1 ordered by d_digits[position] (positions with
 * equal digits keep their order); d_bucket_counts[256] = elements per digit. */
SL_API int  sl_partition_by_digit(sl_ctx* ctx, int64_t n, const uint8_t* d_digits, int64_t* d_perm,
                           int64_t* d_bucket_counts, uint32_t* d_counts);
/* d_rows_out[r] = d_rows_in[d_perm[r]] for rows of `words` 8-byte words. */
SL_API int  sl_gather_rows(sl_ctx* ctx, int64_t count, int words, const int64_t* d_perm,
                    const int64_t* d_rows_in, int64_t* d_rows_out);

/* One row of SL_ADAPTIVE_ROW_WORDS words per cell of [lo,hi): vbits(V), flat index, decrease and
 * threshold(x, tau = 1) = -|L_v(x)|_1 (1 + L_f(x)) from the records of a sweep run with tau = 1
 * (d_records: [hi-lo][record_stride], columns 0 and 1), the refinement N(x) and the flags the loop
 * starts from: d_prior_bits = NULL (can_shrink: the initial set, lyapunov.py:498-505) or the
 * previous safe set with d_prior_ref = the previous refinement (NULL: 1 on safe cells) (:506-510). */
#define SL_ADAPTIVE_ROW_WORDS 6
SL_API int  sl_adaptive_pack(sl_ctx* ctx, int64_t lo, int64_t hi, const double* d_values,
                      const double* d_records, int record_stride, const uint64_t* d_init_bits,
                      const uint64_t* d_prior_bits, const int64_t* d_prior_ref, int64_t* d_rows);
/* d_dest[i] = number of splitter keys (d_splitters[s].key, from sl_select_*) <= row i's key: the rank
 * that owns the row's position in the sorted order. */
SL_API int  sl_adaptive_dest(sl_ctx* ctx, int64_t count, const int64_t* d_rows,
                      const sl_select_state* d_splitters, int nsplit, uint8_t* d_dest);
/* keys[i] = vbits of row i, vals[i] = i: the input of sl_sort_pairs. */
SL_API int  sl_adaptive_sort_keys(sl_ctx* ctx, int64_t m, const int64_t* d_rows, uint64_t* d_keys,
                           int64_t* d_vals);
/* Judge the batches of the m rows at sorted positions [pos0, pos0 + m) (pos0 a multiple of batch;
 * d_order[q] = row of position pos0 + q): d_info[b] = {passes, bound, stop, refine_bound} as in
 * lyapunov.py:537-582, *d_first_break = smallest global batch index that ends the loop (INT64_MAX:
 * none; MIN it over the ranks). */
SL_API int  sl_adaptive_analyse(sl_ctx* ctx, int64_t m, int64_t pos0, int64_t batch,
                         const int64_t* d_rows, const int64_t* d_order, double tau,
                         double safety_factor, int64_t max_refinement, int32_t* d_info,
                         int64_t* d_first_break);
/* d_out_rows[row] = {flat index, safe, refinement} after the loop ended in batch b_star. */
SL_API int  sl_adaptive_apply(sl_ctx* ctx, int64_t m, int64_t pos0, int64_t batch,
                       const int64_t* d_rows, const int64_t* d_order, const int32_t* d_info,
                       double tau, double safety_factor, int64_t b_star, int64_t* d_out_rows);
/* {index, safe, refinement} rows of cells of [lo,hi) -> this range's mask words and refinement
 * array; the initial set is kept (lyapunov.py:601-606); *d_safe_count = bits set. */
SL_API int  sl_adaptive_scatter(sl_ctx* ctx, int64_t lo, int64_t hi, int64_t m,
                         const int64_t* d_out_rows, const uint64_t* d_init_bits,
                         uint64_t* d_safe_bits, int64_t* d_refinement, int64_t* d_safe_count);

/* ---- get_safe_sample / perturb_actions (lyapunov.py:609-797): the glue between the safe set and
 * the point evaluations (sl_eval_points) ------------------------------------------------------------ */
/* d_states[i] = index_to_state(d_indices[i]) on the model's grid (functions.py:714-731). */
SL_API int  sl_index_to_state(sl_ctx* ctx, int64_t count, const int64_t* d_indices, double* d_states);
/* Row i*nperturb + k = [state_i, clip(action_i + perturbation_k, limits)] (lyapunov.py:634-647);
 * d_limits [m][2] may be NULL (no clipping). */
SL_API int  sl_perturb_pairs(sl_ctx* ctx, int64_t count, int d, int m, const double* d_states,
                      const double* d_actions, int nperturb, const double* d_perturbations,
                      const double* d_limits, double* d_pairs);
/* utilities.unique_rows (:496-516) orders rows by memcmp of their raw bytes: d_keys[q] = byte-swapped
 * word `column` of row d_order[q] (NULL: q) - sort by it with sl_sort_pairs, last column first. */
SL_API int  sl_rows_sort_key(sl_ctx* ctx, int64_t count, int words, int column, const int64_t* d_rows,
                      const int64_t* d_order, uint64_t* d_keys);
/* d_flags[q] = 1 when row d_order[q] equals row d_order[q-1] bit for bit (drop it). */
SL_API int  sl_rows_duplicate_flags(sl_ctx* ctx, int64_t count, int words, const int64_t* d_rows,
                             const int64_t* d_order, uint8_t* d_flags);
/* bound_i = sum_j std_ij and inside_i = V(mean_i) + sum_j L_v(mean_i)_j std_ij < c_max
 * (lyapunov.py:716-726); lv_cols = 1 or d. */
SL_API int  sl_sample_bounds(sl_ctx* ctx, int64_t count, int d, int lv_cols, const double* d_std,
                      const double* d_lv, const double* d_value, double c_max, double* d_bound,
                      uint8_t* d_inside);
/* d_inout[i] &= safe_set[state_to_index(point_i)] (lyapunov.py:762-766, functions.py:733-752);
 * d_safe_bits = the mask words of the WHOLE grid. */
SL_API int  sl_state_membership(sl_ctx* ctx, int64_t count, const double* d_points,
                         const uint64_t* d_safe_bits, uint8_t* d_inout);
/* d_out[0] = first index of the largest d_values[i] among rows with d_mask[i] != 0 (NULL: all), NaN
 * counting as largest (np.argmax, lyapunov.py:783, 789), -1 if there is none; d_out[1] = rows seen. */
SL_API int  sl_argmax_masked(sl_ctx* ctx, int64_t count, const double* d_values, const uint8_t* d_mask,
                      int64_t* d_out);
/* discrete_policy_optimization with a safety constraint (reinforcement_learning.py:266-278): d_best[i]
 * = np.argmax_a of d_q[i][a] with the actions that are not allowed at vertex i counted as -inf (first
 * maximiser wins, NaN largest, nothing allowed -> 0).  d_allowed_bits[a * words_per_action + (i >> 6)]
 * bit (i & 63): action a may be taken at vertex i - e.g. the `negative` words of one sl_lyap_sweep
 * per action with that action as the policy (NULL: no constraint).  The [count, A] table of action
 * values stays on the device. */
SL_API int  sl_argmax_rows_masked(sl_ctx* ctx, int64_t count, int n_actions, const double* d_q,
                           const uint64_t* d_allowed_bits, int64_t words_per_action, int32_t* d_best);

/* get_lyapunov_region (lyapunov.py:59-139): the region around the node `start` (flat index on the
 * model's grid) that the reference's priority-queue flood of the function values visits before it
 * reaches the grid boundary or has to descend - computed as a minimax-distance fixpoint.
 *   d_values [nindex] the function on the grid (sl_values), d_work [nindex] scratch (the distances),
 *   d_region [nindex] out: 1 inside; *sweeps_out (may be NULL) relaxation passes used. */
SL_API int  sl_lyapunov_region(sl_ctx* ctx, const double* d_values, int64_t start, double* d_work,
                        uint8_t* d_region, int* sweeps_out);

/* Bit mask <-> byte mask helpers for the bool[N] safe_set of the reference (lyapunov.py:187). */
SL_API int  sl_bits_to_bytes(sl_ctx* ctx, int64_t n, const uint64_t* d_bits, uint8_t* d_bytes);
SL_API int  sl_bytes_to_bits(sl_ctx* ctx, int64_t n, const uint8_t* d_bytes, uint64_t* d_bits);
/* np.where(safe_set) (lyapunov.py:729, the first step of get_safe_sample): the flat indices of the set
 * bits of a mask of n cells, ascending.  Two calls, because the caller sizes d_indices by the count:
 *   sl_bits_count      d_block_counts [ceil(ceil(n/64)/256)] and d_offsets [that + 1] are scratch it fills
 *                      (set bits per 16 384 cells, their exclusive prefix sums); *total_out (HOST) = number
 *                      of set bits - one 8-byte copy and a stream synchronisation;
 *   sl_bits_to_indices d_indices [total] out, with the d_offsets of the count call.
 * Bits of the last word beyond n are ignored. */
SL_API int  sl_bits_count(sl_ctx* ctx, int64_t n, const uint64_t* d_bits, uint32_t* d_block_counts,
                          int64_t* d_offsets, int64_t* total_out);
SL_API int  sl_bits_to_indices(sl_ctx* ctx, int64_t n, const uint64_t* d_bits, const int64_t* d_offsets,
                               int64_t* d_indices);

/* ---- dynamic programming (reinforcement_learning.py:65-140, 213-279) --------------------- */
/* One Jacobi sweep over vertices [lo,hi) of the value grid (auxiliary grid #0):
 *   q(i,a) = r(x_i,u_a) + gamma * V_old(mean f(x_i,u_a))
 * n_actions == 0: u = policy(x_i) (value_iteration, :135-140).
 * n_actions  > 0: u_a = h_actions[a] (row-major [n_actions][m]); writes max_a q and the first
 *                 arg-max (discrete_policy_optimization, :266-279); d_q (may be NULL) gets all q.
 *   d_v_new [hi-lo], d_argmax [hi-lo] (may be NULL), d_stats[2] = {max_i |v_new_i - table_i|,
 *   sum_i (v_new_i - V(x_i))^2} with V(x_i) interpolated as in reinforcement_learning.py:130-133;
 *   the sum (the Bellman error of the current policy, :116-133) is produced for n_actions == 0
 *   only and is 0 otherwise. */
SL_API int  sl_bellman_sweep(sl_ctx* ctx, int64_t lo, int64_t hi, int n_actions, const double* h_actions,
                      double* d_v_new, int32_t* d_argmax, double* d_q, double* d_stats);

/* ---- exact policy evaluation: V = r + gamma P V ------------------------------------------ *
 * sl_policy_operator: the rows of vertices [lo,hi) of the value grid for the current policy -
 * successor = dynamics mean at (x_i, policy(x_i)) located in the value triangulation exactly as
 * sl_bellman_sweep(n_actions = 0) locates it.  Column-major ELL, K = d + 1 entries per row:
 *   d_cols [K][hi-lo] vertex indices, d_w [K][hi-lo] weights (negated for a value spec with
 *   `negate`), d_r [hi-lo] rewards, d_stats[2] = {rows with a negative barycentric weight,
 *   kappa = gamma * max_i sum_k |w_ik|}.  Grids of 1 to 4 dimensions, at most 2^31 - 1 vertices.
 * sl_value_solve: solves (I - gamma P) v = r for any ELL operator of n rows, k <= 16 entries
 *   (cols in [0, n)), d_v = start on entry, on return the iterate whose residual is reported.
 *   Stops when ||r + gamma P v - v||_inf <= tol * ||r||_inf (r = 0: v = 0), when an iterate is not
 *   finite (residual_inf = +inf: diverging, kappa > 1) or when the next step would exceed
 *   max_matvecs operator applications, residuals included (converged = 0; not an error).  method SL_SOLVE_GMRES: restarted GMRES(restart),
 *   a cycle whose true residual is above kappa^steps times the cycle's start is followed by
 *   `restart` Jacobi steps from the better iterate (kappa < 1 only); SL_SOLVE_JACOBI: the
 *   fixed-point iteration v <- r + gamma P v alone.  bound = residual_inf / (1 - kappa) bounds
 *   ||v - v*||_inf when kappa < 1 (+inf otherwise).  Deterministic: no atomics. */
enum sl_solve_method { SL_SOLVE_GMRES = 0, SL_SOLVE_JACOBI = 1 };
typedef struct sl_value_solve_stats {
    int64_t iterations;           /* Arnoldi steps + Jacobi steps                                  */
    int64_t matvecs;              /* operator applications, residuals included                     */
    int64_t cycles, jacobi_cycles;   /* restart cycles / of them safeguard Jacobi cycles (gmres)   */
    double residual_inf, bound, kappa;
    int32_t converged, reserved;
} sl_value_solve_stats;
SL_API int  sl_policy_operator(sl_ctx* ctx, int64_t lo, int64_t hi, int32_t* d_cols, double* d_w,
                               double* d_r, double* d_stats);
SL_API int  sl_value_solve(sl_ctx* ctx, int64_t n, int k, const int32_t* d_cols, const double* d_w,
                           const double* d_r, double gamma, double* d_v, double tol, int64_t max_matvecs,
                           int restart, int method, sl_value_solve_stats* out);

/* Successor cache of sl_bellman_sweep.  The next state of (vertex, action) - and where it falls in the
 * value grid: rectangle, unit-cell simplex, barycentric weights - does not depend on the value table
 * (reinforcement_learning.py:89-104; the table enters at :101 only), and a value-iteration loop
 * repeats the sweep with the same dynamics and action set.  The first max sweep (n_actions > 0) over
 * a range therefore keeps the located successors on the device (8 d + 5 bytes per pair: 6.2 GB for
 * 64^4 vertices x 9 actions); later max sweeps over the same range with the same h_actions - and
 * policy-evaluation sweeps (n_actions == 0) whose table policy takes one of those actions at every
 * vertex - gather and combine from it.  Their results are bit-identical to the uncached kernels'.
 * The cache is dropped by whatever changes a successor: sl_model_set with another grid / dynamics
 * description, sl_gp_set_head[_kernel], sl_gp_append_point, sl_gp_configure with another head count,
 * sl_tri_set(slot 0); sl_tri_set_table, the reward, gamma and the policy may change freely (a policy
 * table overwritten in place: announce it with sl_policy_touch, the select arrays are per policy).
 *   max_bytes < 0: default budget (a quarter of the device's memory); 0: no cache (frees it);
 *   otherwise the largest allocation allowed - a sweep whose cache would not fit recomputes. */
SL_API int  sl_successor_cache_configure(sl_ctx* ctx, int64_t max_bytes);
typedef struct sl_successor_cache_stats {
    int64_t bytes, max_bytes;     /* allocated / allowed                                         */
    int64_t lo, hi;               /* vertex range of the cached sweep                            */
    int32_t valid, n_actions;     /* 1: the next matching sweep is served from the cache         */
    int64_t fills, hits, policy_hits;   /* sweeps that filled it / max sweeps / policy sweeps served */
} sl_successor_cache_stats;
SL_API int  sl_successor_cache_info(sl_ctx* ctx, sl_successor_cache_stats* out);

/* ---- evaluation at arbitrary points (Function.__call__, lyapunov.py:265-288, 324-376) ------ */
enum sl_eval_what {
    SL_EVAL_VALUE = 1,      /* V(x)                    out [n][1]                  */
    SL_EVAL_POLICY = 2,     /* policy(x)               out [n][m]                  */
    SL_EVAL_DYNAMICS = 3,   /* per-point record        out [n][2+2d] =             */
    SL_EVAL_DECREASE = 4,   /*   [v_decrease_bound, threshold, mean f[d], error[d]] (both selectors) */
    SL_EVAL_LV = 5,         /* L_v(x)                  out [n][lv_cols]            */
    SL_EVAL_GRADIENT = 6    /* dV/dx(x), signed        out [n][d]  (SL_V_POLYNOMIAL only)  */
};
SL_API int  sl_eval_points(sl_ctx* ctx, int what, int64_t n, const double* d_points /* [n][d] */,
                    double* d_out);

/* ---- closed-loop rollouts (utilities.py:519-583 compute_trajectory, examples/utilities.py:654-686
 * compute_roa) ----------------------------------------------------------------------------- *
 * sl_rollout advances the trajectories [lo, hi) by `steps` steps of x <- f(x, policy(x)) under the
 *   model of sl_model_set, the state held in registers between steps (one thread per trajectory).
 *   d_start NULL: trajectory i starts at grid point i (GridWorld.all_points: np.linspace, the last
 *     point of an axis is its upper limit), hi <= the number of grid cells;
 *   d_start [hi - lo][d]: explicit start states (the grid of the model is not used);
 *   d_state [hi - lo][d]: the end states; may be d_start itself (continue a rollout in place);
 *   d_traj NULL or [steps][hi - lo][d]: the state after every step, step-major;
 *   d_actions NULL or [steps][hi - lo][m]: the action of every step (policy of the state before it).
 *   The horizon is cut into launches of steps_per_launch steps with the state carried in d_state
 *   (0: the library chooses from hi - lo so that a launch stays near a second); the results do not
 *   depend on it.  steps = 0 copies the start states.
 *   Policies: LINEAR, CONST, TRI (table slot 1); NETWORK runs step by step (its actions of a step
 *   become a per-trajectory table, as in the sweeps); a per-vertex TABLE is defined for one step
 *   only (steps > 1: SL_ERR_INVALID).  SL_DYN_GP: SL_ERR_UNSUPPORTED (step the mean through
 *   sl_eval_points instead).
 * sl_rollout_mask: bit i of d_bits (ceil(n / 64) words, bits past n zero) = ||x_i - e||_2 <= tol
 *   for the states d_state [n][d] (any d up to SL_MAX_STATE_DIM; no model needed) - the rooted sum
 *   of squares as np.linalg.norm adds it, NaN is outside; *d_count (may be NULL) = number of set
 *   bits.  h_equilibrium NULL: the origin.                                                       */
SL_API int  sl_rollout(sl_ctx* ctx, int64_t lo, int64_t hi, const double* d_start, int steps,
                    int steps_per_launch, double* d_state, double* d_traj, double* d_actions);
SL_API int  sl_rollout_mask(sl_ctx* ctx, int64_t n, int d, const double* d_state,
                    const double* h_equilibrium /* [d] */, double tol, uint64_t* d_bits, int64_t* d_count);

/* ---- discounted returns of the closed loop (examples/utilities.py:522-545 reward_rollout) ------ *
 * sl_reward_rollout sums, for the trajectories [lo, hi) under the model of sl_model_set,
 *     d_sum[i] = sum_t d_weights[t] * reward([x_t, policy(x_t)]),   x_{t+1} = f(x_t, policy(x_t))
 *   sequentially from 0.0 (product rounded, then added: no contraction), with the model's `reward`
 *   (kind SL_V_QUADRATIC on [x, u]), and stops as the reference does: after the FIRST step t at
 *   which max over all trajectories of |d_weights[t] * reward| < tol (that term is included), for
 *   every trajectory at once, else after `horizon` terms.  A NaN term never satisfies the test.
 *   d_weights [horizon] on the device: the caller's discount ** t.
 *   d_start as for sl_rollout (NULL: the grid points); d_sum [hi - lo] out; d_state [hi - lo][d]
 *   scratch and out: the state after the dynamics step that follows the last summed term (may be
 *   d_start).  *h_steps (host, may be NULL) = number of terms summed, *h_converged = 1 when the
 *   test stopped the loop.
 *   One thread keeps a trajectory's state and sum in registers for the steps of a launch; the
 *   per-step maxima are read once per launch, and the launch that contains the stopping step is
 *   run once more from its inputs, cut there, so the sums are those of the sequential loop
 *   whatever steps_per_launch is (0: the library chooses, 32 at most; never more than 128).
 *   Policies, SL_DYN_GP and the per-vertex TABLE: as for sl_rollout (NETWORK: step by step).    */
SL_API int  sl_reward_rollout(sl_ctx* ctx, int64_t lo, int64_t hi, const double* d_start, int horizon,
                    const double* d_weights, double tol, int steps_per_launch, double* d_sum,
                    double* d_state, int64_t* h_steps, int* h_converged);

/* ---- the posterior mean of GP dynamics as a deterministic model (functions.py:209-230
 * UncertainFunction.to_mean_function) --------------------------------------------------------- *
 * The model's dynamics must be SL_DYN_GP with its heads configured (sl_gp_configure); any other kind:
 * SL_ERR_UNSUPPORTED (the deterministic kinds belong to sl_rollout / sl_reward_rollout).  The mean is
 *     prior(z) + sum_heads sum_j k(z, x_j) alpha'_j,  z = [x, u]
 * one training point at a time in the operations and order of the Bellman sweeps' successor and of
 * sl_action_gradient's d_next: O(n p) per point, no triangular product, no variance.
 * sl_gp_mean_points: d_mean [n][d] = the mean at the explicit rows d_inputs [n][d + m] (d, m: the
 *   model's; the policy is not evaluated).  One thread per row.
 * sl_rollout_mean: sl_rollout's contract word for word - ranges, grid cells or explicit start
 *   states, step-major d_traj / d_actions, steps = 0, steps_per_launch (0: chosen from (hi - lo) x
 *   training points so that a launch stays near a second), the policies (TRI needs slot 1, a per-vertex
 *   TABLE one step only, NETWORK step by step) - with the GP mean as f.
 * sl_reward_rollout_mean: sl_reward_rollout's signature and contract (weights table, global stopping
 *   rule, the launch holding the stopping step run once more cut there, *h_steps, *h_converged) with
 *   the GP mean as f.
 * All three are deterministic: the same inputs give the same bits.                                */
SL_API int  sl_gp_mean_points(sl_ctx* ctx, int64_t n, const double* d_inputs /* [n][d + m] */,
                    double* d_mean /* [n][d] */);
SL_API int  sl_rollout_mean(sl_ctx* ctx, int64_t lo, int64_t hi, const double* d_start, int steps,
                    int steps_per_launch, double* d_state, double* d_traj, double* d_actions);
SL_API int  sl_reward_rollout_mean(sl_ctx* ctx, int64_t lo, int64_t hi, const double* d_start, int horizon,
                    const double* d_weights, double tol, int steps_per_launch, double* d_sum,
                    double* d_state, int64_t* h_steps, int* h_converged);

/* ---- training a LyapunovNetwork (examples/lyapunov_function_learning.ipynb cells 25 and 30: the
 * two optimizer.minimize(..., var_list=lyapunov_function.parameters)) -------------------------- *
 * Both calls work on the network of sl_network_set alone (no sl_model_set needed); d is the width
 * of the point rows and must be the network's input width, at most SL_MAX_STATE_DIM as in the sweeps.
 * Without a network, with m <= 0 or with another d they return SL_ERR_INVALID.
 * sl_nn_param_grad: for every layer l the [out_l][in_l] matrix
 *     G_l = sum_{i < m} d_coeff[i] * dV(p_i)/dK_l,   p_i = d_points [m][d],
 *   concatenated, row-major, unpadded - the layout sl_network_set takes h_kernels in - into
 *   d_grad_kernels.  FP64 on the matrix cores; every workgroup adds its points into a slice of a
 *   scratch area the context owns and a second kernel adds the slices in a fixed order (no atomics):
 *   two calls with the same inputs return the same bits.  (The step from the layer kernels
 *   [W^T W + eps I ; W'] to the variables W, W' is the caller's: dW = W (G_top + G_top^T),
 *   dW' = G_bottom.)
 * sl_nn_loss: the losses of a batch of m samples and the coefficients that turn them into a
 *   gradient through sl_nn_param_grad, with V from the matrix-core evaluation of the sweeps.
 *   SL_NN_LOSS_ROA (cell 30): states d_states [m][d], successors d_next [m][d], labels l_i in {0, 1}
 *     (d_labels_or_targets [m], as doubles), class weights w_i (d_class_weights [m]):
 *       classifier_i = w_i max(-(2 l_i - 1)(safe_level - V(x_i)), 0)
 *       decrease_i   = l_i max(V(x_i+) - V(x_i), 0) / (V(x_i) + eps)     (denominator: a constant)
 *       objective    = mean_i (classifier_i + lagrange * decrease_i)
 *     d_losses[3] = the means {objective, classifier, decrease}; d_coeff [2 m] = d objective / d V(x_i)
 *     then d objective / d V(x_i+), each already divided by m; d_points (may be NULL) [2 m][d] = the
 *     point list [x; x+] those coefficients belong to.
 *   SL_NN_LOSS_ABS (cell 25): objective = mean_i |V(x_i) - target_i| with the targets in
 *     d_labels_or_targets; d_next and d_class_weights are NULL, the three scalars unused;
 *     d_losses = {objective, objective, 0}, d_coeff [m] = sign(V(x_i) - target_i) / m, d_points [m][d].
 *   max(., 0) and |.| have derivative 0 at the kink (as TensorFlow's gradients have). */
enum sl_nn_loss_kind { SL_NN_LOSS_ABS = 1, SL_NN_LOSS_ROA = 2 };
SL_API int  sl_nn_param_grad(sl_ctx* ctx, int64_t m, int d, const double* d_points, const double* d_coeff,
                    double* d_grad_kernels);
SL_API int  sl_nn_loss(sl_ctx* ctx, int kind, int64_t m, int d, const double* d_states, const double* d_next,
                    const double* d_labels_or_targets, const double* d_class_weights, double safe_level,
                    double lagrange, double eps, double* d_losses, double* d_coeff, double* d_points);

/* ---- policy gradients of future_values (reinforcement_learning.py:65-114; the
 * optimizer.minimize(-reduce(rl.future_values(states)), var_list=rl.policy.parameters) of
 * examples/inverted_pendulum.ipynb cells 9/12 and safe_learning/tests/test_rl.py:29-77), without the
 * Lyapunov penalty.  The chain rule is cut at the action: Q(x, u) = r([x, u]) + gamma V(mu([x, u])),
 *   d sum_i w_i Q(x_i, pi(x_i)) / d theta = sum_i sum_a (w_i dQ/du_a(x_i)) d pi_a(x_i) / d theta.
 * sl_action_gradient: under the model of sl_model_set (policy, dynamics, quadratic reward, value table
 *   in slot 0, gamma) d_grad [n][m] = dQ/du at the points d_points [n][d] (NULL: the first n grid points
 *   of the model, as the Bellman sweeps generate them) and the actions d_actions [n][m] (NULL: u =
 *   policy(x); a network policy goes through a per-point action table as in the sweeps); d_q [n] (may
 *   be NULL) = Q, d_next [n][d] (may be NULL) = the successor mu.
 *     dQ/du_a = [(P + P^T) z]_{d+a} + gamma sum_k c_k dmu_k/du_a
 *   c = gradient of the value table's simplex at the successor, the simplex located as the table's
 *   evaluation locates it; with `project` coordinate k of c counts only while lo_k <= mu_k <= hi_k (the
 *   gradient of tf.minimum(tf.maximum(x, lo), hi), functions.py:1485).  SL_DYN_LINEAR: the action columns of
 *   the matrix; SL_DYN_GP: the prior-mean columns plus sum_j alpha'_jk dk(x_j, z)/du_a of the head that
 *   owns column k, for RBF heads and every sum-of-products description.  The Euler dynamics
 *   (SL_DYN_PENDULUM, SL_DYN_CARTPOLE): SL_ERR_UNSUPPORTED.  One thread per point.
 * sl_policy_param_grad: for the network of sl_policy_network_set (no sl_model_set needed; d = its input
 *   width, at most SL_MAX_STATE_DIM) d_grad = sum_i sum_o d_coeff[i][o] d pi_o(p_i)/d theta for every
 *   kernel and bias, concatenated in the order W_0, b_0, W_1, b_1, ..., W_out (W_l [in][out] row-major;
 *   only the layers that have a bias contribute one) - the order sl_policy_network_set stores them in.
 *   pi = output_scale h_L; activation derivatives as TensorFlow's (relu: 1 for a pre-activation > 0, else
 *   0).  The outer products run on the matrix cores with the points as the reduction dimension, every
 *   workgroup adds into its own slice of context scratch and a second kernel adds the slices in ascending
 *   order: no atomics, the same bits at every call.
 * sl_tri_param_grad: for the table of slot `slot` (sl_tri_set; its grid, simplices and `project`, not
 *   its values) d_grad [nindex][cols] (vertex v) = sum of d_coeff[i][:] w_ik over all (i, k) with
 *   simplex_k(p_i) = v, weights and simplices as the table's evaluation computes them; vertices that no
 *   point touches get 0.  The (vertex, contribution) pairs are ordered with sl_sort_pairs and every run is
 *   added in point order: no atomics, the same bits at every call.  n (d + 1) < 2^31. */
SL_API int  sl_action_gradient(sl_ctx* ctx, int64_t n, const double* d_points, const double* d_actions,
                    double* d_grad, double* d_q, double* d_next);
SL_API int  sl_policy_param_grad(sl_ctx* ctx, int64_t n, int d, const double* d_points, const double* d_coeff,
                    double* d_grad);
SL_API int  sl_tri_param_grad(sl_ctx* ctx, int slot, int64_t n, const double* d_points, const double* d_coeff,
                    double* d_grad);

/* ---- the Lyapunov penalty of future_values, differentiated (reinforcement_learning.py:107-112; the
 * rl.future_values(tf_states, lyapunov=lyapunov) of examples/inverted_pendulum.ipynb cell 17).  Under the model
 * of sl_model_set of a LYAPUNOV context (policy, GP dynamics, Lyapunov function, L_v, L_f, tau), with z = [x, u]:
 *   C(x, u) = V_L(mu) - V_L(x) + sum_k L_k(mu) e_k + |L(x)|_1 (1 + L_f(x)) tau,   e_k = beta sqrt(var_h(z))
 *   dC/du_a = sum_j [g_j(mu) + sum_k dL_k/dmu_j(mu) e_k] dmu_j/du_a + sum_k L_k(mu) beta dvar_h/du_a / (2 sqrt(var_h))
 *   dvar_h/du_a = dk(z, z)/du_a - 2 a^T b_a,   a = L^-1 k_x,  b_a = L^-1 dk_x/du_a
 * d_grad [n][m] = dC/du at the points d_points [n][d] (NULL: the first n grid points) and the actions d_actions
 * [n][m] (NULL: u = policy(x), evaluated once); d_constraint [n] (may be NULL) = C; d_terms [n][2 + 2 d] (may be
 * NULL) = the record of SL_EVAL_DECREASE: decrease bound, threshold (-|L(x)|_1 (1 + L_f) tau), mean, error.
 * g = grad V_L: (P + P^T) mu for a quadratic, the simplex gradient for a table (negated with it, masked per
 * coordinate where the table projects); dL/dmu: sign(.) G for the two linear kinds (sign(0) = 0), 0 for a
 * constant and for the gradient kinds over a table.  sqrt(var) is not clamped.  The triangular products run on
 * the matrix cores from the A fragments the heads hold, in batches through context scratch; no atomics, the
 * same bits at every call and for every split of the points over calls.
 * SL_DYN_GP only: the Euler and the linear dynamics, and SL_V_NETWORK, return SL_ERR_UNSUPPORTED. */
SL_API int  sl_decrease_gradient(sl_ctx* ctx, int64_t n, const double* d_points, const double* d_actions,
                    double* d_grad, double* d_constraint, double* d_terms);

/* ---- actor-critic with a NeuralNetwork value function (examples/reinforcement_learning_pendulum.ipynb cells
 * 16, 31, 34, 48; examples/reinforcement_learning_cartpole.ipynb cell 15): with u = pi(x), x+ = f(x, u), z = [x, u]
 *   target = stop_gradient(r(z) + gamma V(x+))
 *   value objective  = reduce |V(x) - target|          (minimised over the value network's parameters)
 *   policy objective = reduce (r(z) + gamma V(x+))      (maximised over the policy's parameters)
 * The context's one network slot belongs to the policy (sl_policy_network_set), so both calls are stateless about
 * the value network: nlayers, h_dims [nlayers + 1], h_activations, h_has_bias (may be NULL: none) and output_scale
 * as sl_policy_network_set takes them (widths <= 64, at most SL_MAX_NN_LAYERS layers), and d_params = ONE device
 * array of the parameters in the order sl_policy_network_set packs its own: W_0, b_0, W_1, b_1, ..., W_l [in][out]
 * row-major, a bias only for the layers that have one.  The caller owns d_params.
 * sl_critic_batch: under the dynamics (SL_DYN_PENDULUM, SL_DYN_CARTPOLE with their action tangent carried through
 *   the ten Euler sub-steps, SL_DYN_LINEAR), the quadratic reward and gamma of sl_model_set - its value slot is
 *   ignored - for the n states d_states [n][d] and actions d_actions [n][m] (explicit: the caller evaluates the
 *   policy once, e.g. sl_eval_points, so every policy kind and a saturation work), and a value network d -> 1:
 *     d_next [n][d] (may be NULL) = x+, bit for bit the successor of sl_eval_points(SL_EVAL_DYNAMICS)
 *     d_value [n] = V(x),  d_q [n] = q = r + gamma V(x+)
 *     d_dq_du [n][m] (may be NULL): dq/du_a = [(P + P^T) z]_{d+a} + gamma sum_k g_k dx+_k/du_a, g = dV/dx at x+ by
 *       the transposed chain (activation derivatives as sl_policy_param_grad: relu' = 1 for a pre-activation > 0)
 *     d_coeff [n] (may be NULL) = w sign(V(x) - q), sign(0) = 0, w = 1/n (SL_REDUCE_MEAN) or 1 (SL_REDUCE_SUM):
 *       d value objective / d V(x_i) with the target held constant
 *     d_sums [2] = {sum_i |V(x_i) - q_i|, sum_i q_i}, unscaled
 *   One sample per thread; workgroups write partial sums to context scratch and a second kernel adds them in
 *   ascending order: no atomics, the same bits at every call.  SL_DYN_GP: SL_ERR_UNSUPPORTED (sl_action_gradient
 *   serves GP models with a value table).  n == 0, a width above 64, another output width than 1, and a network
 *   or Euler model whose dimensions are not the model's: SL_ERR_INVALID.
 * sl_dense_param_grad: d_out = sum_i sum_o d_coeff[i][o] d net_o(p_i)/d theta for the network of the arguments,
 *   flat in the order of d_params (d = its input width, at most SL_MAX_STATE_DIM; d_points [n][d], d_coeff
 *   [n][outputs]): the kernel of sl_policy_param_grad on a description built from the arguments - for the same
 *   network the two calls return identical bits.  No sl_model_set needed. */
enum sl_reduction { SL_REDUCE_MEAN = 0, SL_REDUCE_SUM = 1 };
SL_API int  sl_critic_batch(sl_ctx* ctx, int nlayers, const int32_t* h_dims, const int32_t* h_activations,
                    const int32_t* h_has_bias, double output_scale, const double* d_params, int64_t n,
                    const double* d_states, const double* d_actions, int reduction, double* d_next,
                    double* d_value, double* d_q, double* d_dq_du, double* d_coeff, double* d_sums);
SL_API int  sl_dense_param_grad(sl_ctx* ctx, int nlayers, const int32_t* h_dims, const int32_t* h_activations,
                    const int32_t* h_has_bias, double output_scale, const double* d_params, int64_t n, int d,
                    const double* d_points, const double* d_coeff, double* d_out);

/* ---- sample paths of a Gaussian process on a discretization (sample_gp_function, functions.py:1586-1662) and
 * the dense FP64 linear algebra behind them.  Device buffers belong to the caller unless marked h_; matrices are
 * row-major with a leading dimension.  Limits: N <= SL_GP_SAMPLE_MAX_N points, k <= SL_GP_SAMPLE_MAX_K columns,
 * p <= SL_MAX_INPUT_DIM, n <= SL_GP_SAMPLE_MAX_TRAIN observations (SL_ERR_UNSUPPORTED above them); N = 1 and
 * k = 1 work.  The calls use the context's scratch area and nothing else of it: the model, the GP heads, the
 * tables and the caches stay as they are.  No atomics: the same input gives the same bits at every call.
 * sl_gp_posterior_cov: GPRCached.build_predict with full_cov=True (functions.py:438-448) at the N points d_Z
 *   [N][p], with the explicit inverse factor this engine uses everywhere: a = h_Linv K(h_X, Z) on the matrix
 *   cores, d_mean [N] = a^T h_alpha + Z h_prior (h_prior [p] or NULL), d_cov [N][ld] = K(Z, Z) - a^T a + jitter I
 *   (a^T a on the matrix cores; the reference's 1E-8 is the caller's jitter).  The lower triangle is computed and
 *   mirrored: d_cov equals its transpose bit for bit.  h_X [n][p], h_Linv [n][n], h_alpha [n] and h_kernel as
 *   sl_gp_set_head_kernel takes them (one output column; a plain RBF is a one-leaf description); n = 0: the prior.
 * sl_cholesky: in-place lower Cholesky factor of d_A [N][ld] (its lower triangle is read), blocked 64 wide: the
 *   diagonal block is factored by one workgroup in LDS, the block rows below it are solved against it by
 *   substitution, the rest loses panel x panel^T on the matrix cores.  The strict upper triangle is zero
 *   afterwards.  A pivot that is not > 0 (a NaN included) ends the factorization: *h_info (may be NULL) = its
 *   1-based index (0 on success) and the call returns SL_ERR_INVALID; the matrix is then partly factored.  The
 *   index travels in a device word that every later kernel of the call reads before it does anything.
 * sl_tri_solve: d_B [N][k] = L^-1 d_B (transpose = 0) or L^-T d_B, block by block: one right-hand side per lane
 *   against the diagonal block, the other block rows updated on the matrix cores.
 * sl_tri_mult: d_out [N][k] = d_mean + L d_Zn (d_mean [N] or NULL; d_out must not be d_Zn), the sum over
 *   ascending k: the sample values for standard normal d_Zn.
 * sl_gp_sample_eval: d_out [M][k] = d_points h_prior + K(d_points, d_D) d_Alpha for d_points [M][p], d_D [N][p],
 *   d_Alpha [N][k]: D and Alpha are streamed through LDS and the sum over j is taken in ascending order, so a
 *   point's result does not depend on M or on the launch shape. */
#define SL_GP_SAMPLE_MAX_N 16384
#define SL_GP_SAMPLE_MAX_K 1024
#define SL_GP_SAMPLE_MAX_TRAIN 4096
SL_API int  sl_gp_posterior_cov(sl_ctx* ctx, int n, int p, const double* h_X, const double* h_Linv,
                    const double* h_alpha, const sl_gp_kernel* h_kernel, const double* h_prior, int64_t N,
                    const double* d_Z, double jitter, double* d_mean, double* d_cov, int64_t ld);
SL_API int  sl_cholesky(sl_ctx* ctx, int64_t N, double* d_A, int64_t ld, int32_t* h_info);
SL_API int  sl_tri_solve(sl_ctx* ctx, int64_t N, int64_t k, const double* d_L, int64_t ld, int transpose,
                    double* d_B);
SL_API int  sl_tri_mult(sl_ctx* ctx, int64_t N, int64_t k, const double* d_L, int64_t ld, const double* d_Zn,
                    const double* d_mean, double* d_out);
SL_API int  sl_gp_sample_eval(sl_ctx* ctx, const sl_gp_kernel* h_kernel, const double* h_prior, int p, int64_t N,
                    const double* d_D, int64_t k, const double* d_Alpha, int64_t M, const double* d_points,
                    double* d_out);

/* ---- hyper-parameters of GP regression: the log marginal likelihood and its gradient (gpflow 0.4.0
 * GPR.build_likelihood; GPRCached.compute_log_likelihood / log_likelihood_gradient / optimize).  With the residuals
 * h_R = Y - m(X) [n][dout] (the columns share the kernel), K = k(h_X, h_X) + noise_variance I = L L^T, B = K^-1 R and
 * W = B B^T - dout K^-1:
 *   *h_lml = -1/2 sum(R o B) - dout sum_i log L_ii - n dout / 2 log 2 pi
 *   h_grad_variance [SL_KERNEL_MAX_FACTORS][SL_MAX_INPUT_DIM], h_grad_inv_ls (the same shape): d lml / d theta =
 *     1/2 sum_ij W_ij dK_ij / d theta for theta = variance[q] / inv_lengthscales[q] of every factor of the
 *     description (entries that are zero in the description keep a zero derivative; at most 32 entries may be
 *     non-zero, SL_ERR_UNSUPPORTED above), *h_grad_noise = 1/2 tr W.  All three may be NULL: then only the value is
 *     computed, and nothing of order n^3 runs beyond the factorization.
 * Stateless like the calls above: the context's scratch area, and device buffers the call allocates and frees.
 * K is formed by sl_gp_posterior_cov without observations, factored by sl_cholesky (a pivot that is not > 0:
 * *h_info (may be NULL) = its 1-based index, SL_ERR_INVALID), B and L^-1 come from sl_tri_solve, K^-1 = L^-T L^-1
 * from the matrix cores, and the sum over (i, j) from one workgroup per lower 64 x 64 tile, the tiles added in
 * ascending order.  No atomics: the same input gives the same bits at every call.  n = 0: 0 and a zero gradient;
 * n > SL_GP_SAMPLE_MAX_TRAIN: SL_ERR_UNSUPPORTED. */
SL_API int  sl_gp_likelihood(sl_ctx* ctx, int n, int p, int dout, const double* h_X, const double* h_R,
                    const sl_gp_kernel* h_kernel, double noise_variance, double* h_lml, double* h_grad_variance,
                    double* h_grad_inv_ls, double* h_grad_noise, int32_t* h_info);

/* ---- multi-GPU collectives directly on RCCL ----------------------------- *
 * For callers without torch.distributed (the Python package issues the same exchanges through
 * torch.distributed, backend "nccl" = RCCL).  One communicator per context, one rank per GPU; every
 * call is asynchronous on the context's stream.  RCCL is bound at run time: on a system without
 * librccl.so the calls return SL_ERR_UNSUPPORTED.
 *   sl_comm_unique_id: rank 0 creates the 128-byte id and hands it to the other ranks out of band.
 *   sl_allreduce_result: the per-shard record of sl_lyap_sweep / sl_lyap_finalize_dev becomes the record
 *     of the whole grid IN PLACE: lexicographic min of `fail`, lexicographic max of `last_safe`
 *     and `max_key`, sums of the counters (the reductions of lyapunov.py:512-606 over shards).
 *   sl_allgather: value-table shards of equal size after a Bellman sweep
 *     (reinforcement_learning.py:135-140); sl_allreduce_max_f64: its residual;
 *   sl_allreduce_sum_u64: the radix-select histograms of sl_select_hist.                        */
#define SL_COMM_ID_BYTES 128
SL_API int  sl_comm_unique_id(unsigned char* id_out /* [SL_COMM_ID_BYTES] */);
SL_API int  sl_comm_init(sl_ctx* ctx, const unsigned char* id /* [SL_COMM_ID_BYTES] */, int rank, int world);
SL_API int  sl_comm_destroy(sl_ctx* ctx);
SL_API int  sl_allreduce_result(sl_ctx* ctx, sl_sweep_result* d_result);
SL_API int  sl_allgather(sl_ctx* ctx, const void* d_send, void* d_recv, int64_t bytes_per_rank);
SL_API int  sl_allreduce_sum_u64(sl_ctx* ctx, uint64_t* d_values, int64_t count);
SL_API int  sl_allreduce_max_f64(sl_ctx* ctx, double* d_values, int64_t count);

/* ---- diagnostics -------------------------------------------------------------------------- */
/* D = A(16x4) * B(4x16) through v_mfma_f64_16x16x4_f64 with this library's fragment maps. */
SL_API int  sl_debug_mfma(sl_ctx* ctx, const double* h_a, const double* h_b, double* h_d);
/* v_mfma_f64_4x4x4_4b_f64 on per-lane operands (nwaves x 64 values each); mode 0: plain, 1..4:
   cbsz = 2, abid = mode - 1 (not a block broadcast for FP64).  Pins the fragment layout in the
   tests. */
SL_API int  sl_debug_mfma4(sl_ctx* ctx, int nwaves, const double* h_a, const double* h_b,
                    const double* h_c, int mode, double* h_d);
/* Sustained FP64 rate probes: which = 0 MFMA, 1 VALU FMA, 2 both interleaved.
 * h_out[3] = {TFLOP/s, sustained shader clock in MHz, shader cycles per MFMA slot per SIMD}. */
SL_API int  sl_debug_fp64_rate(sl_ctx* ctx, int which, int iters, double* h_out);
/* The last two stages of sl_gp_likelihood alone (the sum over the tiles and its reduction) on a B [n][dout] and a
 * K^-1 [n][n] from the host (its lower triangle is read): the gradient tables as sl_gp_likelihood fills them. */
SL_API int  sl_debug_gp_lml_grad(sl_ctx* ctx, int n, int p, int dout, const double* h_X, const double* h_B,
                    const double* h_Kinv, const sl_gp_kernel* h_kernel, double* h_grad_variance,
                    double* h_grad_inv_ls, double* h_grad_noise);
/* The scaled training inputs X / lengthscales of an uploaded GP head as the kernels read them,
 * h_xs [p][n] (row q = input dimension q): lets the tests compare an incrementally extended head
 * (sl_gp_append_point) with a fresh upload bit for bit. */
SL_API int  sl_debug_gp_inputs(sl_ctx* ctx, int head, double* h_xs);
/* The scratch area of sl_nn_param_grad / sl_nn_loss (in the context's scratch buffer, which sl_eval_points
 * uses too) lies between two guard zones that every such call writes in front of its kernels, one directly
 * before the first and one directly behind the last double its kernels own: *h_bytes = the size of the
 * area of the last such call (0: none yet, or the front zone is damaged), *h_guards_intact = 1 when the
 * kernels of that call wrote neither in front of nor behind the area.  Synchronises the stream. */
SL_API int  sl_debug_nn_train_scratch(sl_ctx* ctx, int64_t* h_bytes, int* h_guards_intact);

#ifdef __cplusplus
}
#endif
#endif /* SL_HIP_H */
