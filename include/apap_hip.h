/*
 * apap_hip.h - C ABI of libapap_hip.so, the MI355X (gfx950) engine for the APAP
 * moving-DLT path of Enigmatisms/cvx_proj.
 *
 * The reference has no FFI layer: its boundary for this path is the Python surface
 * of class APAP in pyviz/apap.py and the helpers of pyviz/apap_utils.py, consumed only
 * by apap.py's __main__ (apap.py:238-265).  Every entry point below names the
 * reference interface it stands in for.  A maintainer binds them with ctypes; the
 * binding is shown in INTEGRATION.md and shipped as cvx_proj_amd/_native.py.
 *
 * Conventions
 *  - Plain C types only.  All arrays are row-major and caller-owned; the library
 *    never keeps a pointer after a call returns.
 *  - Every function that returns int returns APAP_OK (0) or one of the APAP_ERR_*
 *    codes; apap_last_error() then gives a thread-local human-readable message.
 *    The reference signals the same conditions with Python exceptions
 *    (numpy.linalg.LinAlgError from apap.py:165-166,203; IndexError from
 *    apap.py:207,209-210; ValueError from the shape unpacking at apap.py:129-130).
 *  - "Host" entry points take host pointers and are synchronous: inputs are copied
 *    to the selected GPU, the kernels run, outputs are copied back before return.
 *  - "_device" entry points take DEVICE pointers (hipMalloc'ed by the caller, or a
 *    torch tensor's data_ptr()) and a hipStream_t passed as void* (NULL = the
 *    default stream).  They only enqueue work; the caller synchronises.  They are
 *    what bench.py and the multi-GPU driver use to keep data resident in HBM.
 *  - Every compute entry point takes an apap_ctx* first (NULL = defaults): options, profiling
 *    and the device-buffer pool live there, not in the process (section "context" below).
 *  - There is no CPU fallback.  Without a usable gfx950 device every compute entry
 *    point fails with APAP_ERR_NO_DEVICE.
 */
#ifndef APAP_HIP_H
#define APAP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APAP_OK 0
#define APAP_ERR_INVALID_ARG 1 /* bad pointer / size (reference: ValueError on unpack)       */
#define APAP_ERR_NO_DEVICE 2   /* no HIP device, or device index out of range                */
#define APAP_ERR_HIP 3         /* a HIP runtime call failed; message has hipGetErrorString   */
#define APAP_ERR_SINGULAR 4    /* exact-zero pivot in a 3x3 inverse (reference: LinAlgError) */
#define APAP_ERR_INDEX 5       /* mesh edges do not cover the canvas (reference: IndexError) */
#define APAP_ERR_WORKSPACE 6   /* caller-provided workspace too small                        */

/* Bits of the device status word (the int *d_status of the resident entry points).  Kernels only OR bits into it, so a
 * caller zeroes it before the calls whose findings it wants.  The host-buffer calls turn it into an error code, testing
 * the bits in this order: SINGULAR -> APAP_ERR_SINGULAR, INDEX -> APAP_ERR_INDEX, UNPREPARED -> APAP_ERR_INVALID_ARG. */
#define APAP_STATUS_SINGULAR 1   /* a cell's 3x3 inverse met an exact-zero pivot (reference: LinAlgError)        */
#define APAP_STATUS_INDEX 2      /* mesh edges do not cover the canvas (reference: IndexError)                 */
#define APAP_STATUS_UNPREPARED 4 /* a gather on a warp workspace without lookup tables for this mesh / canvas */
#define APAP_STATUS_NO_CONVERGENCE 8 /* the spectral eigen-solver hit its restart cap: the best Ritz vector is kept */
/* Bits of the M-step (apap_model_solve*, apap_spectral_em*).  status_to_code above does not test them; the M-step's own entry
 * points decode them (see there). */
#define APAP_STATUS_MODEL_DEGENERATE 16     /* fewer than 4 selected matches, or a rank-deficient reduced system: H is NaN */
#define APAP_STATUS_MODEL_NO_CONVERGENCE 32 /* the interior-point method hit its iteration cap: the best iterate is kept */

/* Doubles per keypoint in the device point table (see apap_host_build_table). */
#define APAP_TABLE_STRIDE 32
/* Doubles in the de-normalisation block: inv(C2), C1, inv(N2), N1 (3x3 row-major each). */
#define APAP_DENORM_DOUBLES 36
/* Doubles per cell in the padded inverse-homography buffer the warp kernel reads. */
#define APAP_HINV_STRIDE 10

/* Solver variants (APAP_OPT_SOLVER_VARIANT).  All produce the same float32 grids on the golden
 * vectors; they differ in the summation order of the 30 moment sums.  With APAP_OPT_MOMENTS = 24: AUTO / MFMA = one
 * 16x16x4 + two 4x4x4_4b instructions per step, MFMA4 / MFMA4X2 = six 4x4x4_4b; VALU is refused. */
#define APAP_VARIANT_AUTO 0
#define APAP_VARIANT_VALU 1 /* one lane per cell, fp64 FMA accumulation            */
#define APAP_VARIANT_MFMA 2 /* v_mfma_f64_16x16x4_f64 accumulation, table via LDS  */
#define APAP_VARIANT_MFMA4 3   /* v_mfma_f64_4x4x4_4b_f64, 16 cells per wave          */
#define APAP_VARIANT_MFMA4X2 4 /* v_mfma_f64_4x4x4_4b_f64, 32 cells per wave share B  */

/* Eigen-solvers of K2 (APAP_OPT_EIGEN_SOLVER). */
#define APAP_EIGEN_AUTO 0              /* = inverse iteration with Jacobi fallback          */
#define APAP_EIGEN_JACOBI 1            /* cyclic Jacobi sweeps only                         */
#define APAP_EIGEN_INVERSE_ITERATION 2 /* LDL^T inverse iteration; Jacobi for cells without a
                                          spectral gap and rank-deficient systems            */

/* Kernel slots of apap_ctx_profile_read. */
#define APAP_PROF_ASSEMBLE 0 /* K1: weighted moment sums A^T W^2 A      */
#define APAP_PROF_EIGEN 1    /* K2: eigen-solve + de-normalise          */
#define APAP_PROF_INVERT 2   /* per-cell 3x3 inverse (+ lookup table)   */
#define APAP_PROF_LUT 3      /* canvas row/column -> cell lookup table  */
#define APAP_PROF_WARP 4     /* K3: backward warp gather                */
#define APAP_PROF_EQ_HIST 5  /* E1: per-channel histogram               */
#define APAP_PROF_EQ_APPLY 6 /* E2: table rebuild + mapping             */
#define APAP_PROF_RANSAC 7   /* R1-R3: hypotheses, scoring, selection   */
#define APAP_PROF_SPECTRAL 8 /* spectral weights: set-up, Lanczos, finish */
#define APAP_PROF_SLOTS 9

/* ABI generation.  Generation 2 put `apap_ctx *` first in every compute entry point while keeping the
 * symbol names of generation 1: a caller built against the old header would still link and then pass a
 * float* where the context goes.  Such a caller must refuse to run: check apap_abi_version() ==
 * APAP_ABI_VERSION once after loading (cvx_proj_amd/_native.py does); a generation-1 library does not
 * export the symbol at all.  Bump on any change of an existing signature. */
#define APAP_ABI_VERSION 6
#define APAP_ABI_VERSION_STRING "0.6"

/* ---------------------------------------------------------------- diagnostics --- */
const char *apap_last_error(void);
const char *apap_version(void);
int apap_abi_version(void);
/* Number of visible HIP devices; 0 when there is none (never an error). */
int apap_device_count(void);

/* -------------------------------------------------------------------- context --- */
/* The library keeps NO process-wide mutable state (the reference's class is re-entrant: all of
 * its state is on `self`, apap.py:22-32).  Every compute entry point takes an `apap_ctx *` as its
 * first argument; NULL means "the built-in defaults, no profiling" and is always valid.  A context
 * carries the options below, the HIP events of its profiling, and the pool of device buffers its
 * host-buffer calls reuse.  One context must not be used from two threads at once; different
 * contexts (and NULL) are independent - NULL-context host-buffer calls share one pool and are
 * serialised on it. */
typedef struct apap_ctx apap_ctx;
#define APAP_OPT_SOLVER_VARIANT 0 /* APAP_VARIANT_*; default AUTO (= MFMA)                              */
#define APAP_OPT_EIGEN_SOLVER 1   /* APAP_EIGEN_*; default AUTO                                         */
#define APAP_OPT_CAREFUL 2        /* 1 (default): cells whose eigen-gap is below 1e-3 of the trace, and every
                                     cell when n < 5, are re-solved from the weighted 2n x 9 rows (Givens QR +
                                     one-sided Jacobi) as apap.py:159-161 does; 0: normal equations only    */
#define APAP_OPT_PROFILE 3        /* 1: bracket every kernel with HIP events (apap_ctx_profile_read)     */
#define APAP_OPT_WANT_WAVES 4     /* tuning: waves K1 aims at before it stops splitting the keypoints     */
#define APAP_OPT_WARP_ROWS 5      /* canvas rows per wave of K3: 1 (default) = chosen from the size of the launch (4 for one
                                     4K canvas and for the fused stitch, 6 for an 8K canvas, 8 for batches of many
                                     canvases); 2, 4, 5, 6, 8 = that many; 0 = the flat-order kernel.  Same canvas bytes in
                                     every form                                                                             */
#define APAP_OPT_WEIGHT_CHUNK_KB 6 /* device staging of the optional weight tensor, KiB (default 1 GiB)   */
#define APAP_OPT_FUSED_MAX_CELLS 7 /* tuning: meshes of up to this many cells (x batch) take the fused K1 + K2
                                      launch when the variant is AUTO (default 4096; 0 = never)             */
#define APAP_OPT_WARP_FAST 8       /* 1 (default): K3 decides a pixel from a float32 estimate of its source coordinate
                                      and takes the exact float64 sequence only where the estimate is within its error
                                      bound of an integer (same canvas, byte for byte); 0: float64 for every pixel    */
#define APAP_OPT_OVERLAP_PCIE 9    /* 0 (default): apap_local_warp / apap_local_stitch make one copy up, one kernel, one copy
                                      down.  1: they pin the caller's buffers for the call (hipHostRegister; buffers the caller already page-locked -
                                      hipHostMalloc, its own registration - are taken as they are) and overlap the
                                      image upload, the warp (in row bands) and the canvas download on three streams.  For
                                      callers that REUSE their image / canvas buffers: the first uses of a buffer pay 8-26 ms of
                                      pinning and mapping (4K pair), every later call saves ~15 %                              */
#define APAP_OPT_PLAN_CELLS 10      /* 0 (default): the solve picks its kernel (fused small-mesh launch or K1 + K2) and its
                                      keypoint splits from THIS call's cells x batch.  c > 0: as for ONE pair of c cells,
                                      whatever the call holds - a shard of a mesh (cvx_proj_amd/dist.py) then sums every
                                      cell's keypoints in the order the whole mesh would on one GPU: the same bits for any
                                      number of ranks, at the price of fewer, larger blocks per GPU                      */
#define APAP_OPT_MOMENTS 11         /* 30 (default): K1 sums the 30 distinct entries of A^T W^2 A with the reference's
                                      float32-ROUNDED DLT products kept verbatim (apap.py:103-119): grids bit-identical to the
                                      reference's.  24 (opt-in): the 24 sums of the EXACT products (SURVEY.md section 8a:
                                      [[S0,0,Sx],[0,S0,Sy],[Sx,Sy,Sr]]) - a quarter less matrix-pipe work in K1, a fifth less
                                      slab traffic; NOT bit-identical: one float32 ulp in a few per cent of a grid's entries
                                      on BASELINE's configurations (tests/test_gpu_moments24.py), where gamma^2 = 0.25 floors
                                      every weight.  Off them (gamma ~ 0, small sigma) the sums' rounding moves H by up to
                                      ~ eps x the cell's condition number: far more than one ulp on ill-conditioned cells, still
                                      within that bound (tests/test_gpu_weight_range.py).
                                      The device entry points then expect the table of apap_host_build_table24 (a table of the
                                      other layout gives NaN grids); the host-buffer entry points build the right one themselves.
                                      No fused small-mesh launch, no VALU variant in this mode                             */
#define APAP_OPT_WEIGHTS_F32 12     /* 0 (default).  1 (opt-in, honoured with APAP_OPT_MOMENTS = 24 only): K1 evaluates w^2 in
                                      float32 (v_sqrt_f32, v_exp_f32) instead of float64; the sums stay float64.  With
                                      w^2 = 2^x, x = -2 log2(e) d / sigma^2, the relative error of a w^2 is at most
                                      (6 |x| + 4) 2^-24 + 2 log2(e) ln(2) c / sigma^2 (c: what the float32 rounding of the
                                      vertex and keypoint coordinates moves d by, <= 2^-24 (|v| + |s|) per axis): ~2e-7 only
                                      near x = 0, 5e-5 at x = -126; below x = -126 w^2 is 0 (v_exp_f32 flushes subnormals).
                                      So K2 re-solves every cell whose trace is below 2^-40 from float64 weights (the careful
                                      path, with APAP_OPT_CAREFUL = 1): the cells kept on float32 weights are those whose
                                      normal matrix is within the bound above (oracle/weight_spec.py, tests/test_weight_spec.py).
                                      Their H then differs from the default's by up to ~ bound x the cell's condition number;
                                      with gamma^2 flooring every weight (BASELINE's gamma = 0.5, sigma = 100: |x| <= 2) that
                                      is the class of MOMENTS = 24 alone (one float32 ulp here and there).  gamma >= 1 makes
                                      every weight gamma: this chain then clamps at 1 (gamma^2 overflows float32 at 1.8e19)  */
#define APAP_OPT_PLAN_SLOTS 13      /* 0 (default): the blocks of K1's 16x16x4 kernel that the device keeps resident at once are
                                      asked of the device (once per context).  A single pair (batch = 1) whose J = tiles x
                                      splits blocks are more than these S slots and fewer than 2 S is launched as S blocks, J - S
                                      of them carrying TWO 64-cell tiles of one keypoint split, so that none waits for a second
                                      round.  s > 0: plan that pairing as for s resident slots (a large s switches it off).
                                      It moves K1's block-to-tile mapping (and, in a paired launch, the issue priority of its
                                      waves) and nothing else: splits, workspace size, the
                                      moment slabs and the grids are the same bits for every value                        */
#define APAP_OPT_WARP_SAMPLING 14   /* APAP_SAMPLING_NEAREST (0, default): a canvas pixel is source pixel (int(tx), int(ty)), the
                                      reference's truncation (apap.py:211-215).  APAP_SAMPLING_BILINEAR (1): the same float64
                                      coordinate, the same footprint (a pixel is present iff the truncating warp has one there),
                                      sampled from its four neighbours with 5 fractional bits - X = rint(32 tx), taps at
                                      X >> 5 and X >> 5 + 1 clamped to the picture (the border is replicated),
                                      (sum of weight x tap + 512) >> 10 per channel.  Honoured by every warp, stitch, band, batch
                                      and plan entry point and by the panorama.  APAP_OPT_WARP_ROWS and APAP_OPT_WARP_FAST are
                                      ignored under bilinear sampling (one all-float64 strip kernel), and so is
                                      APAP_OPT_OVERLAP_PCIE (the host-buffer warp takes the plain path)                        */
#define APAP_SAMPLING_NEAREST 0
#define APAP_SAMPLING_BILINEAR 1
#define APAP_OPT_COUNT 15
apap_ctx *apap_ctx_create(void);
void apap_ctx_destroy(apap_ctx *ctx); /* frees the pooled device buffers and pending events; NULL is a no-op */
int apap_ctx_set_option(apap_ctx *ctx, int option, int value);
int apap_ctx_get_option(const apap_ctx *ctx, int option, int *value); /* ctx may be NULL: the defaults */
/* K1's short weight chain, a switch of the context beside the option table (which stays as it is: APAP_OPT_COUNT options).
 * 1 (default): K1's 16x16x4 kernel with float64 weights runs a 64-keypoint chunk on a shorter weight chain - the exp table's
 * entry already scaled, no clamp at gamma^2 - where it has proved, from the chunk's keypoints and the bounding box of the
 * block's cells, that the scaling is one the table holds and the clamp is idle.  0: every chunk runs the full chain.  The
 * moment slabs and the grids are the same bits for both values: the switch exists for tests and for A/B measurements.
 * set: ctx must not be NULL, value 0 or 1.  get: ctx may be NULL (the default). */
int apap_ctx_set_short_chain(apap_ctx *ctx, int value);
int apap_ctx_get_short_chain(const apap_ctx *ctx, int *value);
/* Waits for the events recorded since the previous read and returns, per slot, the summed
 * milliseconds and the number of launches. */
int apap_ctx_profile_read(apap_ctx *ctx, float *ms, int *launches);
/* Under APAP_OPT_PROFILE K1's 16x16x4 kernel also counts, per block, the 64-keypoint chunks it ran and how many of them on
 * the short weight chain (apap_ctx_set_short_chain).  Waits for the device, returns both sums since the previous read and
 * clears them; zeros when no such launch was profiled.  (A paired block counts its chunks once, not once per tile.) */
int apap_ctx_profile_k1_chunks(apap_ctx *ctx, unsigned int *short_chunks, unsigned int *chunks);

/* ------------------------------------------------------------ host-only helpers --- */
/* No GPU needed.  They restate, in C and in float32 exactly as numpy evaluates the
 * reference, the once-per-pair set-up that APAP.local_homography performs before its
 * cell loop. */

/* APAP.getNormalize2DPts x2, getConditionerFromPts x2, point_normalize x2
 * (apap.py:35-100,133-140) and the two float32 inverses of apap.py:165-166.
 * src, dst: n x 2 float32.  Outputs (any may be NULL): N1,N2,C1,C2,iC2,iN2 are 3x3
 * float32 row-major; nf1,nf2,cf1,cf2 are n x 2 float32. */
int apap_host_prepare(const float *src, const float *dst, int n, float *N1, float *N2, float *C1,
                      float *C2, float *iC2, float *iN2, float *nf1, float *nf2, float *cf1,
                      float *cf2);

/* APAP.matrix_generate (apap.py:103-119): the 2n x 9 float32 DLT matrix. */
int apap_host_dlt_rows(const float *cf1, const float *cf2, int n, float *aa);

/* The same set-up in the dtype of the keypoints, as the reference's functions run when they are handed float64 points
 * (nothing in apap.py:35-100 casts its argument: float64 keypoints stay float64 until the 3 x 3 matrices and the DLT rows
 * are rounded into float32 arrays, apap.py:53-55,85-87,104-118).  src / dst: n x 2 float32 or float64, each with its own flag
 * (numpy promotes per set).  nf*, cf* come back as float64 (a float32 set's values widened, exactly).  product_f64 of the
 * DLT rows = "one of the two sets was float64": the products -cf2 * cf1 are then float64 products rounded once on the store;
 * with both sets float32 the three *_pts functions give the bits of the float32 functions above. */
int apap_host_prepare_pts(const void *src, int src_f64, const void *dst, int dst_f64, int n, float *N1, float *N2, float *C1,
                          float *C2, float *iC2, float *iN2, double *nf1, double *nf2, double *cf1, double *cf2);
int apap_host_dlt_rows_pts(const double *cf1, const double *cf2, int n, int product_f64, float *aa);
/* the device point table from the DLT rows themselves (`aa`: 2n x 9 float32) and the float64 (or widened) source keypoints */
int apap_host_build_table_rows(const double *src, const float *aa, int n, double *table);

/* Device point table: per keypoint APAP_TABLE_STRIDE doubles -
 *   [0..29]  the 30 distinct entries of r1 r1^T + r2 r2^T, r1/r2 being the point's two
 *            float32 DLT rows (products of float32 values are exact in float64),
 *   [30,31]  the source keypoint (x, y) widened to float64.
 * and the 36-double de-normalisation block. */
int apap_host_build_table(const float *src, const float *cf1, const float *cf2, int n,
                          double *table);
/* The table of APAP_OPT_MOMENTS = 24, from the same DLT rows `aa` (2n x 9 float32) and source keypoints: with p = (x, y, 1)
 * and c = -x', f = -y' as `aa` holds them (aa[k][0..1], aa[2k][8], aa[2k+1][8]), and pp = (xx, xy, x, yy, y, 1) -
 *   [0..5] pp   [6..11] c pp   [12..17] f pp   [18..23] (c^2 + f^2) pp     (float64 products of the float32 values)
 *   [24..27] the rows' own float32 products aa[2k][6], aa[2k][7], aa[2k+1][6], aa[2k+1][7] (the careful path re-solves from
 *            the reference's rows), [28] the layout marker (a quiet NaN), [29] the source keypoint as two float32
 *            (APAP_OPT_WEIGHTS_F32), [30,31] the source keypoint (x, y) as float64. */
int apap_host_build_table24(const double *src, const float *aa, int n, double *table);
int apap_host_build_denorm(const float *iC2, const float *C1, const float *iN2, const float *N1,
                           double *denorm);

/* ------------------------------------------------------ host-buffer entry points --- */

/* APAP.local_homography (apap.py:121-169).
 *   src, dst   n x 2 float32 keypoints (src -> dst)
 *   vertices   mesh_rows x mesh_cols x 2 float64 cell sample points
 *   gamma,sigma  the two scalars of APAP.__init__ (apap.py:22-32)
 *   H_out      mesh_rows x mesh_cols x 9 float32
 *   W_out      NULL, or mesh_rows x mesh_cols x n float64 (the reference's second
 *              return value; 8*n bytes per cell of extra HBM + PCIe traffic)
 *   device     HIP device index, or -1 for the current device */
int apap_local_homography(apap_ctx *ctx, const float *src, const float *dst, int n, const double *vertices,
                          int mesh_rows, int mesh_cols, double gamma, double sigma, float *H_out,
                          double *W_out, int device);
/* The same for keypoints of either dtype (src_f64 / dst_f64: the array holds float64): the set-up then runs as the
 * reference's does on such arrays (apap_host_prepare_pts), and the weights use the float64 source keypoints as they are
 * (apap.py:150: `vertices - src_point` in float64).  apap_local_homography is this call with both flags 0. */
int apap_local_homography_pts(apap_ctx *ctx, const void *src, int src_f64, const void *dst, int dst_f64, int n,
                              const double *vertices, int mesh_rows, int mesh_cols, double gamma, double sigma, float *H_out,
                              double *W_out, int device);

/* The second return value of APAP.local_homography alone (apap.py:144,150-153,169): W_out[c][k] =
 * max(exp(-|vertices[c] - src[k]| / sigma^2), gamma), cells x n float64, for ANY list of `cells` sample points
 * (the whole mesh, or the cells a caller indexes: cvx_proj_amd.apap.LazyWeights).  The reference's own caller
 * never reads this tensor (apap.py:242); computing it on demand keeps its 8 n bytes per cell off the default path. */
int apap_local_weights(apap_ctx *ctx, const float *src, int n, const double *vertices, int cells, double gamma,
                       double sigma, double *W_out, int device);
int apap_local_weights_pts(apap_ctx *ctx, const void *src, int src_f64, int n, const double *vertices, int cells, double gamma,
                           double sigma, double *W_out, int device);

/* APAP.local_warp (apap.py:186-217).
 *   img        img_h x img_w x 3 uint8
 *   Hfwd       mesh_rows x mesh_cols x 9 float32; inverted per cell inside, like
 *              apap.py:201-203 does in place
 *   mesh_w/h   cell edges along x / y (the two rows of get_mesh), n_w / n_h entries
 *   out        final_h x final_w x 3 uint8
 *   Hinv_out   NULL, or mesh_rows x mesh_cols x 9 float32 receiving the inverses (what
 *              the reference leaves in its mutated argument) */
int apap_local_warp(apap_ctx *ctx, const uint8_t *img, int img_h, int img_w, const float *Hfwd, int mesh_rows,
                    int mesh_cols, const double *mesh_w, int n_w, const double *mesh_h, int n_h,
                    int final_w, int final_h, int off_x, int off_y, uint8_t *out, float *Hinv_out,
                    int device);

/* APAP.local_warp for a float64 grid.  The reference inverts the cells in the grid's own dtype
 * (apap.py:201-203: numpy.linalg.inv keeps float64) and multiplies in float64, so a float64 grid is
 * NOT rounded to float32 on the way: Hfwd and Hinv_out are float64 here, everything else is as
 * apap_local_warp. */
int apap_local_warp_f64(apap_ctx *ctx, const uint8_t *img, int img_h, int img_w, const double *Hfwd, int mesh_rows,
                        int mesh_cols, const double *mesh_w, int n_w, const double *mesh_h, int n_h,
                        int final_w, int final_h, int off_x, int off_y, uint8_t *out, double *Hinv_out,
                        int device);

/* The stitch the reference's __main__ keeps commented out (apap.py:258-262), fused into
 * one pass: warp `img` like apap_local_warp, paste `center` (center_h x center_w x 3) at
 * (off_x, off_y) on an empty canvas, uniform_blend (apap_utils.py:75-88) the two.  The
 * centre image must fit the canvas at the offsets (the reference's slice assignment raises
 * otherwise): APAP_ERR_INVALID_ARG. */
int apap_local_stitch(apap_ctx *ctx, const uint8_t *img, int img_h, int img_w, const uint8_t *center, int center_h,
                      int center_w, const float *Hfwd, int mesh_rows, int mesh_cols,
                      const double *mesh_w, int n_w, const double *mesh_h, int n_h, int final_w,
                      int final_h, int off_x, int off_y, uint8_t *out, float *Hinv_out, int device);

/* Same inputs as apap_local_warp; writes the float64 target coordinates (tx, ty) of
 * every canvas pixel (apap.py:211-213) instead of gathering.  coords: final_h x
 * final_w x 2 float64.  For parity tests of the coordinate arithmetic. */
int apap_warp_coords(apap_ctx *ctx, const float *Hfwd, int mesh_rows, int mesh_cols, const double *mesh_w, int n_w,
                     const double *mesh_h, int n_h, int final_w, int final_h, int off_x, int off_y,
                     double *coords, int device);

/* Output stage of apap.py:250-264: per cell H <- inv(H), H /= H[2,2] (float32), then
 * the transposed 3x3 flattened to 9 float64.  H: cells x 9 float32; out: cells x 9. */
int apap_invert_normalize_flatten(apap_ctx *ctx, const float *H, int cells, double *out, int device);

/* uniform_blend (apap_utils.py:75-88) over two h x w x 3 uint8 canvases. */
int apap_uniform_blend(apap_ctx *ctx, const uint8_t *img1, const uint8_t *img2, int h, int w, uint8_t *out,
                       int device);

/* -------------------------------------------------- resident (device) entry points --- */

/* Bytes of scratch apap_solve_device needs for this problem size. */
size_t apap_solve_workspace_bytes(apap_ctx *ctx, int n, int cells);

/* Per-cell weighted DLT + eigen-solve + de-normalisation on resident data.
 *   d_table    n x APAP_TABLE_STRIDE doubles   (apap_host_build_table)
 *   d_vertices cells x 2 doubles
 *   d_denorm   APAP_DENORM_DOUBLES doubles     (apap_host_build_denorm)
 *   d_H        cells x 9 floats (output)
 *   d_work     scratch of apap_solve_workspace_bytes(ctx, n, cells) bytes, 256-byte aligned (as hipMalloc returns it; the
 *              MFMA variant writes it in whole 128-byte lines and refuses another address with APAP_ERR_INVALID_ARG) */
int apap_solve_device(apap_ctx *ctx, const double *d_table, int n, const double *d_vertices, int cells,
                      double gamma, double sigma, const double *d_denorm, float *d_H, void *d_work,
                      size_t work_bytes, void *stream);

/* The same for a BATCH of image pairs with equal n and cell count in one launch
 * (blockIdx.z = pair): d_tables batch x n x 32, d_denorms batch x 36, d_H batch x cells x 9;
 * d_vertices + k * vertices_stride is pair k's mesh (stride in doubles; 0 = one mesh shared
 * by all pairs).  Fills the chip with fewer keypoint splits than `batch` separate calls. */
size_t apap_solve_batch_workspace_bytes(apap_ctx *ctx, int n, int cells, int batch);
int apap_solve_batch_device(apap_ctx *ctx, const double *d_tables, int n, const double *d_vertices, long long vertices_stride,
                            int cells, double gamma, double sigma, const double *d_denorms, float *d_H,
                            int batch, void *d_work, size_t work_bytes, void *stream);

/* The solve of a caller that WARPS NEXT (apap.py:240-243 followed by :186-217 - the reference's own sequence): the same
 * kernels as apap_solve_batch_device with the warp's per-cell set-up riding in the eigen-solve kernel's tail, where it costs
 * a fraction of a launch of its own: every cell leaves, beside its float32 H, its inverse, its float32-estimate record and its
 * exact-path floats in the warp workspace - what APAP_WARP_CELLS would compute from the stored grid, bit for bit (one
 * device function serves both).  The warp that follows runs apap_warp_batch_device(... phases = APAP_WARP_GATHER ...) on that
 * workspace (APAP_WARP_GEOMETRY once per mesh / canvas geometry, before or after).  cells = mesh_rows * mesh_cols; the mesh
 * edges, canvas size and offsets are the warp's.  d_status: the warp's status word (APAP_STATUS_*).  Meshes beyond
 * 4096 edges per axis: APAP_ERR_INVALID_ARG (solve and warp them with the separate entry points). */
int apap_solve_warp_batch_device(apap_ctx *ctx, const double *d_tables, int n, const double *d_vertices, long long vertices_stride,
                                 double gamma, double sigma, const double *d_denorms, float *d_H, int batch, void *d_work,
                                 size_t work_bytes, int mesh_rows, int mesh_cols, const double *d_mesh_w, int n_w,
                                 const double *d_mesh_h, int n_h, int final_w, int final_h, int off_x, int off_y,
                                 void *d_warp_work, size_t warp_work_bytes, int *d_status, void *stream);

/* The weights tensor alone: d_W cells x n doubles. */
int apap_weights_device(apap_ctx *ctx, const double *d_table, int n, const double *d_vertices, int cells,
                        double gamma, double sigma, double *d_W, void *stream);

size_t apap_warp_workspace_bytes(int mesh_rows, int mesh_cols, int final_w, int final_h);

/* Backward warp on resident data.  d_status: the status word (APAP_STATUS_*); zero it
 * before the call.  d_Hinv_out may be NULL. */
int apap_warp_device(apap_ctx *ctx, const uint8_t *d_img, int img_h, int img_w, const float *d_Hfwd, int mesh_rows,
                     int mesh_cols, const double *d_mesh_w, int n_w, const double *d_mesh_h,
                     int n_h, int final_w, int final_h, int off_x, int off_y, uint8_t *d_out,
                     float *d_Hinv_out, void *d_work, size_t work_bytes, int *d_status,
                     void *stream);

/* apap_warp_device for a float64 grid (see apap_local_warp_f64). */
int apap_warp_f64_device(apap_ctx *ctx, const uint8_t *d_img, int img_h, int img_w, const double *d_Hfwd, int mesh_rows,
                         int mesh_cols, const double *d_mesh_w, int n_w, const double *d_mesh_h, int n_h, int final_w,
                         int final_h, int off_x, int off_y, uint8_t *d_out, double *d_Hinv_out, void *d_work,
                         size_t work_bytes, int *d_status, void *stream);

/* apap_warp_device restricted to canvas rows [row_begin, row_begin + row_count): what one
 * rank computes when the warp of ONE pair is sharded over GPUs (cvx_proj_amd/dist.py).
 * d_out_band receives row_count x final_w x 3 bytes. */
int apap_warp_rows_device(apap_ctx *ctx, const uint8_t *d_img, int img_h, int img_w, const float *d_Hfwd, int mesh_rows,
                          int mesh_cols, const double *d_mesh_w, int n_w, const double *d_mesh_h, int n_h,
                          int final_w, int final_h, int off_x, int off_y, int row_begin, int row_count,
                          uint8_t *d_out_band, void *d_work, size_t work_bytes, int *d_status, void *stream);

/* The warp of a BATCH of independent pairs in one set of launches (BASELINE.json config 5: 64 pairs of one size; the
 * reference runs apap.py:186-217 once per pair), and the general form of every warp entry point above.
 * All pairs share the mesh edges, the canvas size and the offsets (pairs of one configuration do); pair k has its own
 *   image   d_imgs + k * img_stride bytes (img_h x img_w x 3; stride 0 = one image for all),
 *   centre  d_centers + k * center_stride bytes, or d_centers = NULL for the plain warp (non-NULL: the fused stitch),
 *   grid    d_Hfwd + k * mesh_rows * mesh_cols * 9 floats (what apap_solve_batch_device writes),
 *   canvas  d_outs + k * out_stride bytes, receiving rows [row_begin, row_begin + row_count) of its canvas,
 *   inverse d_Hinv_out + k * mesh_rows * mesh_cols * 9 floats, when d_Hinv_out is not NULL.
 * grid.z of the kernels is the pair: one set-up launch covers every pair's cells, one gather launch every canvas -
 * 64 pairs fill the chip where one pair's ~9000 waves are 1.45 generations with idle set-up, ramp and tail.
 * `phases`: which steps run on the workspace, any combination of
 *   APAP_WARP_GEOMETRY  canvas row / column -> cell tables: depend on the edges, the canvas size and the offsets only;
 *   APAP_WARP_CELLS     per-cell inverses and the float32 estimate's records: depend on the H grids (and the edges);
 *   APAP_WARP_GATHER    K3, reading what the other two left in the workspace.
 * A caller that warps many grids over one geometry runs GEOMETRY once and CELLS | GATHER per grid; APAP_WARP_ALL is the
 * one-call form.  A GATHER on a workspace whose tables were never built, or were built for another mesh shape / canvas
 * size, touches nothing and sets APAP_STATUS_UNPREPARED in *d_status (the tables carry a stamp of the sizes they were built
 * for).  d_work: apap_warp_batch_workspace_bytes(...) bytes; the layout is private but stable between calls
 * with equal (mesh_rows, mesh_cols, final_w, final_h, batch). */
#define APAP_WARP_GEOMETRY 1
#define APAP_WARP_CELLS 2
#define APAP_WARP_GATHER 4
#define APAP_WARP_ALL 7
size_t apap_warp_batch_workspace_bytes(int mesh_rows, int mesh_cols, int final_w, int final_h, int batch);
int apap_warp_batch_device(apap_ctx *ctx, const uint8_t *d_imgs, long long img_stride, int img_h, int img_w,
                           const uint8_t *d_centers, long long center_stride, int center_h, int center_w,
                           const float *d_Hfwd, int mesh_rows, int mesh_cols, const double *d_mesh_w, int n_w,
                           const double *d_mesh_h, int n_h, int final_w, int final_h, int off_x, int off_y,
                           int row_begin, int row_count, uint8_t *d_outs, long long out_stride, float *d_Hinv_out,
                           int batch, int phases, void *d_work, size_t work_bytes, int *d_status, void *stream);

/* Resident-data twin of apap_local_stitch. */
int apap_stitch_device(apap_ctx *ctx, const uint8_t *d_img, int img_h, int img_w, const uint8_t *d_center, int center_h,
                       int center_w, const float *d_Hfwd, int mesh_rows, int mesh_cols,
                       const double *d_mesh_w, int n_w, const double *d_mesh_h, int n_h, int final_w,
                       int final_h, int off_x, int off_y, uint8_t *d_out, float *d_Hinv_out, void *d_work,
                       size_t work_bytes, int *d_status, void *stream);

/* Coordinates-only twin of apap_warp_device (d_coords: final_h x final_w x 2 doubles). */
int apap_warp_coords_device(apap_ctx *ctx, const float *d_Hfwd, int mesh_rows, int mesh_cols, const double *d_mesh_w,
                            int n_w, const double *d_mesh_h, int n_h, int final_w, int final_h,
                            int off_x, int off_y, double *d_coords, void *d_work, size_t work_bytes,
                            int *d_status, void *stream);

int apap_flatten_device(apap_ctx *ctx, const float *d_H, int cells, double *d_out, int *d_status, void *stream);

int apap_blend_device(apap_ctx *ctx, const uint8_t *d_a, const uint8_t *d_b, int h, int w, uint8_t *d_out, void *stream);

/* ------------------------------------------- callers of the path --- */
/* Pre-processing of apap.py:236-237 = utils.py:85-91 visualize_equalized_hist:
 *   np.stack([cv.equalizeHist(img[..., i]) for i in range(3)], axis=-1)
 * on an interleaved uint8 image of 1..4 channels (h x w x channels); out may alias nothing.
 * cv::equalizeHist (opencv-python 4.6.0.66, absent from this image) is restated from its
 * published algorithm: see oracle/frontend_oracle.py. */
int apap_equalize_hist(apap_ctx *ctx, const uint8_t *img, int h, int w, int channels, uint8_t *out, int device);
size_t apap_equalize_workspace_bytes(int channels);
/* Resident-data form: three kernels on `stream` (histogram; table; mapping).  WORKSPACE
 * CONTRACT: d_work (16-byte aligned, apap_equalize_workspace_bytes(channels) bytes) must be all
 * zero on entry - zero it once after allocating it - and is all zero again, apart from the table
 * at its end, when the call's kernels have run; so back-to-back calls need no memset. */
int apap_equalize_hist_device(apap_ctx *ctx, const uint8_t *d_img, int h, int w, int channels, uint8_t *d_out, void *d_work,
                              size_t work_bytes, void *stream);

/* Seed homography, the contract of baseline_stitch_test.py:42
 *     H, mask = cv.findHomography(src_pts, dst_pts, cv.RANSAC, thresh)
 * src, dst: n x 2 float32.  `iterations` 4-point hypotheses drawn by a counter-based sampler
 * (`seed`), forward reprojection error against thresh, the first hypothesis with the most
 * inliers wins; H_out (9 doubles, row-major, H[8] = 1) is the normalised DLT of the hot path
 * (apap.py:35-119,160-168, all weights 1) re-fitted to its inliers; mask_out: n bytes 0/1.
 * *inliers_out < 4 means no model (cv returns None): H_out is then left untouched.  This is this
 * repository's estimator, not OpenCV's (sampler, adaptive stopping and LM polish differ):
 * oracle/frontend_oracle.py is its specification. */
#define APAP_RANSAC_ITERATIONS 2048
#define APAP_RANSAC_SEED 0x5EEDC0DE5EEDC0DEull
int apap_find_homography_ransac(apap_ctx *ctx, const float *src, const float *dst, int n, double thresh, int iterations,
                                unsigned long long seed, double *H_out, uint8_t *mask_out, int *inliers_out,
                                int device);
size_t apap_ransac_workspace_bytes(int n, int iterations);
/* Device half (no re-fit): d_H_best 9 doubles = the winning 4-point model, d_mask n bytes,
 * d_result 2 ints = {winning hypothesis, its inlier count}.  Points 8-byte aligned. */
int apap_ransac_device(apap_ctx *ctx, const float *d_src, const float *d_dst, int n, double thresh, int iterations,
                       unsigned long long seed, double *d_H_best, uint8_t *d_mask, int *d_result, void *d_work,
                       size_t work_bytes, void *stream);

/* Fundamental matrix from matches, the contract of
 *     F, mask = cv.findFundamentalMat(src_pts, dst_pts, cv.FM_RANSAC, thresh)
 * src (the centre picture's points), dst (the other picture's): n x 2 float32, n >= 8; dst_h^T F src_h = 0, the convention
 * of calculate_M's epipolar score (F @ homo_src, dotted with homo_dst).  `iterations` 8-point hypotheses drawn by the
 * counter-based sampler of the seed homography (`seed`; 8 draws a hypothesis) on coordinates normalised by each picture's
 * bounding box, each reduced by Gaussian elimination with complete pivoting (no rank constraint); a match is an inlier when
 * its squared Sampson distance is <= thresh^2 (pixels); the first hypothesis with the most inliers wins.  F is re-fitted on
 * the device to the winner's inliers (A^T A in one fixed summation order, cyclic Jacobi, rank 2 by a Jacobi SVD), scaled so
 * that max_k |(F src_k)[:2]| = 1 over all n matches - |dst^T F src| is then at most the distance in pixels of dst from the
 * epipolar line of src - and signed so that its first entry of largest magnitude is positive.
 * F_out: 9 doubles, row-major; mask_out: n bytes 0/1; *inliers_out: the winner's count.  Fewer than 8 inliers, or a
 * degenerate scale, is "no model" (cv returns None): F_out is nine NaN and the host-buffer call clears mask_out.
 * thresh >= 0 (inf allowed), 1 <= iterations <= 2^24.  This is this repository's estimator, not OpenCV's (sampler, adaptive
 * stopping and polish differ): tests/fundamental_spec.py is its specification, bit for bit.
 * The batch forms take pair_offset[0 .. n_pairs] (HOST ints, as apap_match_descriptors_batch): pair p holds rows
 * pair_offset[p] .. pair_offset[p + 1] - 1 of src / dst / mask, 1 <= n_pairs <= 65535; F_out 9 doubles and inliers_out one
 * int per pair.  A pair's results are those of its own call; the number of kernel launches does not depend on n_pairs. */
int apap_find_fundamental_ransac(apap_ctx *ctx, const float *src, const float *dst, int n, double thresh, int iterations,
                                 unsigned long long seed, double *F_out, uint8_t *mask_out, int *inliers_out, int device);
int apap_find_fundamental_ransac_batch(apap_ctx *ctx, const float *src, const float *dst, const int *pair_offset, int n_pairs,
                                       double thresh, int iterations, unsigned long long seed, double *F_out, uint8_t *mask_out,
                                       int *inliers_out, int device);
/* Workspace of the resident forms for n_pairs pairs of n_total matches in all (0 for invalid arguments).  Its parts, each
 * rounded up to a multiple of 256 bytes, in this order (every one is written in full by a call, none needs a set-up):
 *     offsets   (n_pairs + 1) ints            the pair table
 *     boxes     n_pairs x 8 doubles           centre x, centre y, scale, extent of src's bounding box, then of dst's
 *     hyps      n_pairs x iterations x 9 doubles   every hypothesis, de-normalised (nine NaN: a zero or non-finite pivot)
 *     winners   n_pairs x 9 doubles           the winning hypothesis
 *     counts    n_pairs x iterations ints     every hypothesis's inliers */
size_t apap_fundamental_workspace_bytes(int n_total, int n_pairs, int iterations);
/* Resident forms: device pointers but pair_offset; d_F 9 doubles a pair (nine NaN: no model), d_mask the winner's inliers
 * (rows as src; not cleared when there is no model), d_result 2 ints a pair = {winning hypothesis, its inlier count}.
 * d_work 256-byte aligned, points and d_F 8-byte aligned.  Five launches on `stream`, timed under APAP_PROF_RANSAC; no
 * wait.  d_F feeds apap_spectral_device / apap_spectral_em_device / apap_spectral_em_batch_device as their d_F. */
int apap_fundamental_device(apap_ctx *ctx, const float *d_src, const float *d_dst, int n, double thresh, int iterations,
                            unsigned long long seed, double *d_F, uint8_t *d_mask, int *d_result, void *d_work, size_t work_bytes,
                            void *stream);
int apap_fundamental_batch_device(apap_ctx *ctx, const float *d_src, const float *d_dst, const int *pair_offset, int n_pairs,
                                  double thresh, int iterations, unsigned long long seed, double *d_F, uint8_t *d_mask,
                                  int *d_result, void *d_work, size_t work_bytes, void *stream);

/* ------------------------------------------------- notch denoising of periodic noise --- */
/* apply_median_filter of pyviz/median_filter.py on uint8 planes of h rows x w columns:
 *     plane = equalizeHist(plane); F = fftshift(fft2(plane))                                    (:130-136)
 *     for i in 2 .. sn - 1: the calls (i, i), (j, i) and (i, j) for j < i with radii (r, 5 r), then (0, i) and (i, 0) with
 *         radii (3, 3 r); a call (a, b) makes four assignments F[D <= r1] = median(F[D <= r2]), D the distance from
 *         (w / 2 +- a spacing, h / 2 +- b spacing), in place and in order                        (:97-126, :143-155)
 *     out = |ifft2(ifftshift(F))|                                                               (:160-162)
 * np.median of complex values orders them by real part, then imaginary part, and returns (a + b) / 2 of the two middle
 * ones for an even count; discs are clipped to the plane, an empty one assigns nothing.  Everything is complex128.  The
 * transform is this library's own (mixed radix 4, 2, 3, 5 Stockham, rows then columns; the inverse columns then rows with
 * the conjugate table, scaled once by the double 1.0 / (h w)); the magnitude is sqrt(re re + im im) of the scaled value, the
 * uint8 output min(255, floor(x + 0.5)).  tests/denoise_spec.py is the specification, byte for byte.
 * Lengths: 5-smooth, APAP_FFT_MIN_LENGTH .. APAP_FFT_MAX_LENGTH each.  1 <= r <= APAP_NOTCH_MAX_R, sn >= 2 and
 * spacing > max(6 r, 5 r + 3): then no write disc meets another centre's read disc, and every distinct centre is
 * evaluated from the spectrum as it was (one block each).  There is no CPU path: ERR_NO_DEVICE without a device. */
#define APAP_FFT_MIN_LENGTH 2
#define APAP_FFT_MAX_LENGTH 4096
#define APAP_NOTCH_MAX_R 6
#define APAP_DENOISE_OUT_F64 0
#define APAP_DENOISE_OUT_U8 1
/* out[2 k], out[2 k + 1] = cos, sin of -2 pi k / n, k = 0 .. n - 1, correctly rounded from extended precision; (1, 0) at
 * k = 0.  Host only: the table the kernels read and the specification reads. */
int apap_fft_twiddles(int n, double *out);
/* 2-D transform of `planes` complex128 planes (interleaved re, im; h x w each).  in == out is allowed.  The resident form's
 * workspace (256-byte aligned) receives the two twiddle tables and, for h > 1024, a turned copy of the planes: columns that
 * long do not fit a strip of four in LDS, so the planes are transposed through LDS tiles, their columns transformed as rows
 * (the same arithmetic) and transposed back - every global access of every pass covers 64 consecutive bytes or the plane's width. */
int apap_fft2(apap_ctx *ctx, const double *in, double *out, int planes, int h, int w, int inverse, int device);
size_t apap_fft2_workspace_bytes(int planes, int h, int w);
int apap_fft2_device(apap_ctx *ctx, const double *d_in, double *d_out, int planes, int h, int w, int inverse, void *d_work,
                     size_t work_bytes, void *stream);
/* The notch step alone, in place, on `planes` SHIFTED spectra (fftshift's layout) of any h, w in 1 .. 4096: one launch. */
int apap_notch_spectrum(apap_ctx *ctx, double *f, int planes, int h, int w, int spacing, int r, int sn, int device);
int apap_notch_spectrum_device(apap_ctx *ctx, double *d_f, int planes, int h, int w, int spacing, int r, int sn, void *stream);
/* The whole chain on n_images pictures of one shape, `channels` (1 .. 4) interleaved channels each, n_images * channels <=
 * 65535 planes.  equalize = 0 skips the equalisation.  out: the pictures' layout, float64 (APAP_DENOISE_OUT_F64) or uint8
 * (APAP_DENOISE_OUT_U8, what apap_corner_detect reads).  The spectrum is kept unshifted; the shift is index arithmetic in
 * the notch kernel.  Launches of the resident form: the equalisation's own per picture, then five whatever the number of
 * planes - forward rows (reads the uint8 plane), forward columns, notch, inverse columns, inverse rows (writes only the
 * magnitude) - or, for h > 1024, seven: the spectrum is transposed once before the column transform and once after the inverse
 * one, and the notch works on the turned copy.  Workspace (256-byte aligned, no contract between calls): the two twiddle
 * tables, planes x h x w complex128 (twice for h > 1024), the equalised pictures, the equalisation's own workspace. */
int apap_notch_denoise(apap_ctx *ctx, const uint8_t *imgs, int n_images, int h, int w, int channels, int equalize, int spacing,
                       int r, int sn, int out_type, void *out, int device);
size_t apap_notch_denoise_workspace_bytes(int n_images, int h, int w, int channels);
int apap_notch_denoise_device(apap_ctx *ctx, const uint8_t *d_imgs, int n_images, int h, int w, int channels, int equalize,
                              int spacing, int r, int sn, int out_type, void *d_out, void *d_work, size_t work_bytes, void *stream);

/* ------------------------------------------------- co-visibility tracks and triangulation --- */
/* get_covid of pyviz/sfm_test.py:79-95 (with has_affinity :23-28) for V views of one centre picture, 1 <= V <=
 * APAP_COVIS_MAX_VIEWS.  View v holds view_offset[v + 1] - view_offset[v] >= 0 observations, the views concatenated
 * (view_offset[0] = 0, at most APAP_COVIS_MAX_POINTS in all: the first-candidate scan is quadratic, a spatial grid for more is
 * out of scope); an observation is a centre-picture point pts[2 g], pts[2 g + 1] (float32) and an index idx[g] into that
 * view's other-picture keypoints.  The reference's sequence is the definition: every observation of view 0 opens a track, in
 * order; every later observation, in order, joins the FIRST track, in track order, whose point q has fabsf(q.x - p.x) < eps
 * and fabsf(q.y - p.y) < eps (float32, strict; NaN matches nothing) and sets that track's column v (a later observation of
 * the same view overwrites an earlier one), or opens a new track at the end.  eps is finite and >= 0; the reference's is 0.1f.
 *   table        n_tracks x V ints: the index seen in each view or -1        track_pts  n_tracks x 2 floats: the founder's point
 *   point_track  one int an observation: the track it ended in               n_tracks   one int
 * table and track_pts are sized for the worst case (as many tracks as observations); rows behind n_tracks are not written.
 * tests/sfm_spec.py is the specification; the kernels (csrc/apap_sfm.hip) equal it bit for bit.  No CPU path.
 *
 * Workspace of the resident form (256-byte aligned, no contract between calls), parts rounded up to 256 bytes, in order:
 *     offsets  (V + 1) ints                     the view table
 *     first    max(n_points, 1) ints            per observation the first earlier in-box position; the resolver moves it on
 *     owner    max(n_points, 1) ints            the position that founded the observation's track
 *     rank     max(n_points, 1) ints            a founder's track
 * apap_covis_workspace_bytes returns 0 for invalid arguments.
 * The resident form takes device pointers but view_offset, allocates nothing and does not wait: one fill and five launches
 * on `stream`.  d_status (zeroed by the caller): APAP_STATUS_COVIS_BOUND is OR-ed in if the resolver's round count reached
 * its structural bound (every undecided observation then opens a track); the host-buffer form returns APAP_ERR_HIP for it. */
#define APAP_COVIS_MAX_VIEWS 8
#define APAP_COVIS_MAX_POINTS 65536
#define APAP_STATUS_COVIS_BOUND 64
size_t apap_covis_workspace_bytes(int n_points, int n_views);
int apap_covis_tracks(apap_ctx *ctx, const float *pts, const int *idx, const int *view_offset, int n_views, float eps, int *table_out,
                      float *track_pts_out, int *point_track_out, int *n_tracks_out, int device);
int apap_covis_tracks_device(apap_ctx *ctx, const float *d_pts, const int *d_idx, const int *view_offset, int n_views, float eps,
                             int *d_table, float *d_track_pts, int *d_point_track, int *d_n_tracks, int *d_status, void *d_work,
                             size_t work_bytes, void *stream);
/* solve_3d_position of pyviz/sfm_test.py:125-136 for many tracks at once, float64: for a track's rays (o_k, d_k) in order
 * A = sum (I - d d^T), p = sum (I - d d^T) o; A = V diag(lam) V^T by cyclic Jacobi; X = V diag(1 / max(lam, 1e-3)) V^T p.
 * The clamp is on every eigenvalue and has no sign rule (the reference scales its last singular value by s / |s|, which is
 * 0 / 0 at exact degeneracy).  Per track: X 3 doubles, lam_min (the smallest eigenvalue before the clamp), n_rays.  A track
 * without rays has X and lam_min NaN and n_rays 0; a non-finite X is stored as three canonical NaN.
 * apap_triangulate_rays: track k owns rays ray_offset[k] .. ray_offset[k + 1] - 1 of origins / dirs (3 doubles a ray).  The
 * host form refuses offsets that do not start at 0 or descend; the resident form reads them on the device and treats a range
 * that is reversed or outside 0 .. n_rays_total as empty.
 * apap_triangulate_tracks: the rays are built from the tracks (covid_3d_optimize :139-167, world_frame_ray_dir of
 * utils.py:188-202): the centre picture's ray through track_pts[k] with camera center_cam first, then for every view v,
 * ascending, whose column holds an index inside 0 .. dst_offset[v + 1] - dst_offset[v] - 1 the ray through that point of
 * dst_pts (float32 pairs, the views concatenated) with camera view_cam[v].  A pixel (u, v) of camera c gives
 * cam = Kinv (u, v, 1), w = (cam_x, cam_z, -cam_y) / |.|, d = R_c w; the ray starts at origins[c].  Kinv 9 doubles, R n_cams x 9,
 * origins n_cams x 3.  A track seen in fewer than min_views >= 1 views (the reference: 2) has no rays.  The resident form
 * takes device pointers but dst_offset and view_cam (they travel in the kernel argument: no workspace), reads the number of
 * tracks from *d_n_tracks (NULL: max_tracks), capped at max_tracks, and writes nothing behind it.  One launch each, no wait. */
int apap_triangulate_rays(apap_ctx *ctx, const double *origins, const double *dirs, const int *ray_offset, int n_tracks, double *X_out,
                          double *lam_min_out, int *n_rays_out, int device);
int apap_triangulate_rays_device(apap_ctx *ctx, const double *d_origins, const double *d_dirs, const int *d_ray_offset, int n_rays_total,
                                 int n_tracks, double *d_X, double *d_lam_min, int *d_n_rays, void *stream);
int apap_triangulate_tracks(apap_ctx *ctx, const int *table, const float *track_pts, int n_tracks, int n_views, const float *dst_pts,
                            const int *dst_offset, const double *Kinv, const double *R, const double *origins, int n_cams,
                            int center_cam, const int *view_cam, int min_views, double *X_out, double *lam_min_out, int *n_rays_out,
                            int device);
int apap_triangulate_tracks_device(apap_ctx *ctx, const int *d_table, const float *d_track_pts, const int *d_n_tracks, int max_tracks,
                                   int n_views, const float *d_dst_pts, const int *dst_offset, const double *d_Kinv, const double *d_R,
                                   const double *d_origins, int n_cams, int center_cam, const int *view_cam, int min_views, double *d_X,
                                   double *d_lam_min, int *d_n_rays, void *stream);

/* ------------------------------------------------- dark-channel dehazing with guided refinement --- */
/* Single-picture dehazing by the dark channel prior (He, Sun, Tang, CVPR 2009) with the guided filter (ECCV 2010) refining
 * the transmission, in exact integers; tests/dehaze_spec.py is the specification, byte for byte.  A picture I is uint8, h x w
 * with 1 (grey) or 3 (BGR) interleaved channels, h, w >= 1, N = h w < 2^31.  Every window is (2 r + 1)^2 with the border
 * replicated; every division is a floor division.
 *     D = window min (radius) of m = min_c I_c                                                   the dark channel, uint8
 *     k = max(1, N / 1000); T = the largest level v with #{D >= v} >= k; among ALL pixels with D >= T the one with the
 *         largest I_0 + I_1 + I_2, the lowest index among equals, gives A; each channel raised to at least 1
 *     n = min(4096, min_c (4096 I_c) / A_c); Dn = window min (radius) of n; p = 4096 - ((omega_q Dn + 128) >> 8)
 *     refine = rho > 0, W = (2 rho + 1)^2, S the box sum of radius rho, G = the grey value of apap_corner_detect:
 *         covN = W S(G p) - S(G) S(p); varN = W S(G G) - S(G)^2; a_q = (4096 covN) / (varN + eps W^2)
 *         b_q = 4096 S(p) - a_q S(G); t = (S(a_q) G W + S(b_q)) / (4096 W^2)            all in int64; rho = 0: t = p
 *     t = clip(t, t0_q, 4096), uint16 with 12 fractional bits
 *     J_c = clip(A_c + (8192 (I_c - A_c) + t) / (2 t), 0, 255)                  round-half-up of A + (I - A) / t
 * radius, refine 0 .. APAP_DEHAZE_MAX_RADIUS; omega_q = rint(256 omega), 0 .. 256; t0_q = max(1, rint(4096 t0)), 1 .. 4096;
 * eps 1 .. 65535 in grey levels squared.  All pictures of a call (1 .. 65535, one shape) share the launches: five, or four
 * without refinement.  The histogram and the selection use integer atomics only: no result depends on a launch or an order.
 * The resident forms take one workspace (256-byte aligned, apap_dehaze_workspace_bytes with the call's refine, or 0 where the
 * entry point has none; contents do not matter, no contract between calls).  No CPU path: ERR_NO_DEVICE without a device.
 * The tile sides of the kernels (tests place pictures at one less, equal and one more): */
#define APAP_DEHAZE_MAX_RADIUS 32
#define APAP_DEHAZE_MIN_TILE_ROWS 16
#define APAP_DEHAZE_MIN_TILE_COLS 128
#define APAP_DEHAZE_AB_TILE_ROWS 16
#define APAP_DEHAZE_AB_TILE_COLS 64
#define APAP_DEHAZE_REC_TILE_ROWS 16
#define APAP_DEHAZE_REC_TILE_COLS 64
#define APAP_DEHAZE_AIR_CHUNK 1024
/* the selection's grid is at most this many blocks: a picture of more than AIR_MAX_BLOCKS x AIR_CHUNK pixels takes them in passes */
#define APAP_DEHAZE_AIR_MAX_BLOCKS 1024
size_t apap_dehaze_workspace_bytes(int n_images, int h, int w, int channels, int refine);
/* dark: n_images x h x w uint8. */
int apap_dark_channel(apap_ctx *ctx, const uint8_t *imgs, int n_images, int h, int w, int channels, int radius, uint8_t *dark, int device);
int apap_dark_channel_device(apap_ctx *ctx, const uint8_t *d_imgs, int n_images, int h, int w, int channels, int radius, uint8_t *d_dark,
                             void *d_work, size_t work_bytes, void *stream);
/* A: n_images x channels uint8. */
int apap_atmospheric_light(apap_ctx *ctx, const uint8_t *imgs, int n_images, int h, int w, int channels, int radius, uint8_t *A, int device);
int apap_atmospheric_light_device(apap_ctx *ctx, const uint8_t *d_imgs, int n_images, int h, int w, int channels, int radius, uint8_t *d_A,
                                  void *d_work, size_t work_bytes, void *stream);
/* t: n_images x h x w uint16, refined (refine > 0) or not, clipped. */
int apap_transmission(apap_ctx *ctx, const uint8_t *imgs, int n_images, int h, int w, int channels, int radius, int omega_q, int t0_q,
                      int refine, int eps, uint16_t *t, int device);
int apap_transmission_device(apap_ctx *ctx, const uint8_t *d_imgs, int n_images, int h, int w, int channels, int radius, int omega_q, int t0_q,
                             int refine, int eps, uint16_t *d_t, void *d_work, size_t work_bytes, void *stream);
/* out: the pictures' layout, uint8 (what apap_corner_detect reads).  t and A as above where the pointer is not NULL. */
int apap_dehaze(apap_ctx *ctx, const uint8_t *imgs, int n_images, int h, int w, int channels, int radius, int omega_q, int t0_q, int refine,
                int eps, uint8_t *out, uint16_t *t, uint8_t *A, int device);
int apap_dehaze_device(apap_ctx *ctx, const uint8_t *d_imgs, int n_images, int h, int w, int channels, int radius, int omega_q, int t0_q,
                       int refine, int eps, uint8_t *d_out, uint16_t *d_t, uint8_t *d_A, void *d_work, size_t work_bytes, void *stream);

/* ------------------------------------------------- spectral match weighting --- */
/* calculate_M of spectral_method.py:66-133, the step every shell driver of the reference runs:
 *     M_ii = match_score_i + epi_weight / (1 + |dst_i^T F src_i|)                              (:104-114)
 *     M_ij = max(4.5 - (|src_i - src_j|^2 - |dst_i - dst_j|^2)^2 / (2 affinity_eps^2), 0)      (:116-124)
 *     U, _, _ = np.linalg.svd(M); segment = |U[:, 0]| / max|U[:, 0]|; segment[segment < 1e-6] = 0  (:125-128)
 *     bool_mask = segment > aff_thresh; ransac_mask *= aff_thresh; ransac_mask[bool_mask] = segment[bool_mask]  (:129-132)
 * M is never stored: its off-diagonal float32 entries (every operation rounded as numpy does) are recomputed inside each
 * fp64 matrix-vector product of a restarted Lanczos iteration (basis of 64, full re-orthogonalisation, start vector
 * 1/sqrt(n)).  U[:, 0] of a symmetric M is the eigenvector of largest |lambda| (M is not positive definite: lambda may be
 * negative).  Converged: |M v - lambda v| <= 1e-13 |lambda|.  Otherwise, after the restart cap, the last Ritz vector is
 * used and APAP_STATUS_NO_CONVERGENCE is reported.
 *   src, dst        n x 2 float32 (cv_to_array: src = kpts_cp[queryIdx], dst = kpts_op[trainIdx])
 *   c_feats, o_feats  n x APAP_SPECTRAL_DIM float32 descriptors, NOT normalised (the call normalises, :109-110)
 *   F               3 x 3 float64, row-major
 *   params          APAP_SPECTRAL_PARAMS doubles, indexed by APAP_SPECTRAL_* below (max_restarts 0 = the default, 30)
 *   Hg_or_null      3 x 3 float32: the initial mask is recompute_matching(Hg) (:35-64), in float32; or NULL and
 *   mask_in_or_null n float32: the initial mask (what match_RANSAC returned).  Both NULL: APAP_ERR_INVALID_ARG (the
 *                   reference's init_ransac=False fails on `None *= float`, :131)
 *   segment_out     n float64;  ransac_mask_out, original_mask_out  n float32
 *   info_out        APAP_SPECTRAL_INFO doubles: lambda, relative gap (|l1| - |l2|) / |l1| of the last tridiagonal (NaN if
 *                   none had two Ritz values), Lanczos steps, status word (APAP_STATUS_NO_CONVERGENCE or 0), restarts,
 *                   last measured |M v - lambda v| / |lambda|
 * The host-buffer call waits for each restart cycle and stops at convergence; it returns APAP_OK also when the cap is hit
 * (the status is in info_out[3]).  n >= 1. */
#define APAP_SPECTRAL_DIM 128
#define APAP_SPECTRAL_EPI_WEIGHT 0
#define APAP_SPECTRAL_AFFINITY_EPS 1
#define APAP_SPECTRAL_AFF_THRESH 2
#define APAP_SPECTRAL_EM_RADIUS 3
#define APAP_SPECTRAL_SCORE_THRESH 4
#define APAP_SPECTRAL_MAX_RESTARTS 5
#define APAP_SPECTRAL_PARAMS 6
#define APAP_SPECTRAL_INFO 6
int apap_spectral_weights(apap_ctx *ctx, const float *src, const float *dst, const float *c_feats, const float *o_feats, int n,
                          const double *F, const double *params, const float *Hg_or_null, const float *mask_in_or_null,
                          double *segment_out, float *ransac_mask_out, float *original_mask_out, double *info_out, int device);
/* Scratch of the resident form: O(n) (about 620 n bytes; the Krylov basis is 512 n of it), no n x n buffer. */
size_t apap_spectral_workspace_bytes(int n);
/* Resident form: every pointer but `params` (host) is a device pointer; d_work 256-byte aligned, points 8-byte aligned.
 * Enqueues the set-up, max_restarts restart cycles and the finish on `stream` without waiting: the launches of the cycles
 * after convergence read the device's `converged` word and return at once.  d_info: APAP_SPECTRAL_INFO doubles;
 * d_status (may be NULL): APAP_STATUS_NO_CONVERGENCE is OR-ed into it when the cap is hit. */
int apap_spectral_device(apap_ctx *ctx, const float *d_src, const float *d_dst, const float *d_c_feats, const float *d_o_feats,
                         int n, const double *d_F, const double *params, const float *d_Hg_or_null,
                         const float *d_mask_in_or_null, double *d_segment, float *d_ransac_mask, float *d_original_mask,
                         double *d_info, int *d_status, void *d_work, size_t work_bytes, void *stream);
/* The dense M itself (n <= 8192: n x n float64, row-major), for the reference's verbose path (plt.imshow(M), :119-126)
 * and for parity tests.  Same inputs as apap_spectral_weights; params' thresholds are not used. */
int apap_spectral_affinity(apap_ctx *ctx, const float *src, const float *dst, const float *c_feats, const float *o_feats, int n,
                           const double *F, const double *params, double *M_out, int device);

/* ------------------------------------------------- M-step and EM loop of the spectral method --- */
/* model_solve of spectral_method.py:165-186 with model.py's solvers, in fp64, without cvxpy:
 *   LMS  (LMSSolver, huber_param <= 1e-2):  min ||A h - rhs||^2                                   (model.py:29-41)
 *   SDP  (SDPSolver(max_iter, du, dv)):     min r + t  s.t.  [[I_2n, P], [P^T, diag(r, r, t)]] >= 0,
 *        P = [A1 h, A2 h, A h - rhs]                                                              (model.py:77-109)
 * A, rhs (float32) and A1, A2 (float64) are built row by row on the device in the reference's dtypes and rounding from the
 * selected matches (weight > the floor, in order).  A tall-skinny QR of K = [A | -rhs | A1's columns 0 3 6 | A2's 1 4 7]
 * (2n x 15, fp64, fixed summation order) reduces the (2n+3)-sized LMI exactly to an 18 x 18 one in (h, r, t); the columns of
 * h are equilibrated by powers of two.  LMS: back-substitution.  SDP: a primal-dual interior-point method (HKM direction,
 * Mehrotra predictor-corrector, 10 x 10 Schur complement system) until tr(S Z) <= 1e-10 (r + t) or the iteration cap.
 * The tail is model.py:50-56: h rounded to float32 with [2, 2] = 1; with swap, inverted (numpy.linalg.inv: fp64 LU, cast
 * to float32) and divided by its [2, 2] in float32.
 *   pts_c, pts_o    n x 2 float32 (kpts_cp[queryIdx].pt, kpts_op[trainIdx].pt)
 *   weights         n float32
 *   params          APAP_MODEL_PARAMS doubles, indexed by APAP_MODEL_* below
 *   H_out           3 x 3 float32, row-major: what SDPSolver.solve / LMSSolver.solve returns
 *   info_out        APAP_MODEL_INFO doubles, indexed by APAP_MODEL_INFO_* below
 * Host-buffer call: H_out and info_out are set to NaN before anything else (a non-NULL pointer); an argument error returns
 * APAP_ERR_INVALID_ARG with them so.  Once the kernels ran both hold their results and the call returns APAP_ERR_INVALID_ARG
 * when APAP_STATUS_MODEL_DEGENERATE is set (H is NaN), APAP_ERR_SINGULAR when the inverse met a zero pivot (numpy:
 * LinAlgError), APAP_OK otherwise, also when the iteration cap was hit (the status word is in
 * info_out[APAP_MODEL_INFO_STATUS]).  n >= 1.
 *
 *   HUBER (LMSSolver, huber_param = M > 1e-2):  min sum_j phi_M(r_j), r = A h - rhs (fp64),
 *        phi_M(r) = r^2 if |r| <= M, 2 M |r| - M^2 otherwise (cvxpy's huber(x, M))                (model.py:36-41)
 * on the same rows as LMS, from the least-squares solution h0: Newton steps on the quadratic piece of the current clipped
 * set (8 x 8 Cholesky, power-of-two column scales) with a halving line search, a majorise-minimise step where that fails,
 * all inside one launch of one workgroup of APAP_MODEL_HUBER_THREADS threads; match i is always summed by thread
 * i mod APAP_MODEL_HUBER_THREADS in ascending order, then one fixed tree, so a call is deterministic.  M travels in the
 * APAP_MODEL_DU slot (the reference's single `param` is either fluc or huber_param); the DV slot is ignored but must be
 * finite.  M not finite or <= 1e-2, or n > 2^20 (one workgroup serves a problem): APAP_ERR_INVALID_ARG before any device
 * is touched.  The info block: OBJECTIVE = f(h) at the returned h, ITERS = the accepted steps, R, T, Z = NaN, and
 *     GAP = (f(h) - D) / f(h) (0 when f(h) = 0),  D = -sum y'^2 / 4 - rhs^T y',
 *     y' = theta (y - A (A^T A)^-1 A^T y),  y = 2 clip(r, -M, M),  theta = min(1, 2 M / max|.|):
 * D bounds the optimum from below for any h (the Fenchel dual, phi*(y) = y^2 / 4 on |y| <= 2 M subject to A^T y = 0), so
 * the gap certifies the returned h whatever the method did.  APAP_STATUS_MODEL_NO_CONVERGENCE is set exactly when GAP is
 * above 1e-10 (the iterate with the lowest f is returned: every accepted step lowers f).  When no row is clipped at h0 the
 * least-squares outputs stay as they are (H byte-identical to LMS, ITERS 0).  Degenerate input behaves as in LMS.
 * apap_spectral_em_batch* and apap_local_model_solve* refuse mode HUBER (APAP_ERR_INVALID_ARG). */
#define APAP_MODEL_LMS 0
#define APAP_MODEL_SDP 1
#define APAP_MODEL_HUBER 2
#define APAP_MODEL_HUBER_THREADS 256 /* the width of the Huber M-step's workgroup                               */
#define APAP_MODEL_MODE 0      /* APAP_MODEL_LMS, APAP_MODEL_SDP or APAP_MODEL_HUBER                            */
#define APAP_MODEL_DU 1        /* SDPSolver's du (model_solve: fluc); HUBER: M                                  */
#define APAP_MODEL_HUBER_M APAP_MODEL_DU
#define APAP_MODEL_DV 2        /* SDPSolver's dv (model_solve: fluc)                                            */
#define APAP_MODEL_FLOOR 3     /* keep the matches with weight > floor (model_solve: 1e-3); -inf keeps them all  */
#define APAP_MODEL_SWAP 4      /* 1: invert and normalise the solution (model.py:53-55)                          */
#define APAP_MODEL_MAX_ITER 5  /* iteration cap; 0 = the default: 80 (SDP, interior point), 100 (HUBER, steps)   */
#define APAP_MODEL_PARAMS 6
#define APAP_MODEL_INFO_OBJECTIVE 0 /* r + t (SDP), ||A h - rhs||^2 (LMS) or f(h) (HUBER)                        */
#define APAP_MODEL_INFO_R 1         /* SDP: r                                                                   */
#define APAP_MODEL_INFO_T 2         /* SDP: t                                                                   */
#define APAP_MODEL_INFO_GAP 3       /* SDP: tr(S Z) / (r + t) of the returned iterate (0 for LMS); HUBER: above   */
#define APAP_MODEL_INFO_ITERS 4     /* SDP: interior-point iterations; HUBER: accepted steps                    */
#define APAP_MODEL_INFO_STATUS 5    /* status word (APAP_STATUS_MODEL_*, APAP_STATUS_SINGULAR)                  */
#define APAP_MODEL_INFO_COUNT 6     /* selected matches                                                          */
#define APAP_MODEL_INFO_Z 7         /* SDP: 9 doubles, the dual 3 x 3 block (order u, v, q): the certificate      */
#define APAP_MODEL_INFO_H 16        /* 8 doubles: h in fp64, before the float32 tail                             */
#define APAP_MODEL_INFO 24
int apap_model_solve(apap_ctx *ctx, const float *pts_c, const float *pts_o, const float *weights, int n, const double *params,
                     float *H_out, double *info_out, int device);
/* Scratch of the resident form for n matches: O(n / 240) 15 x 15 factors, 256-byte multiple. */
size_t apap_model_workspace_bytes(int n);
/* Resident form: every pointer but `params` (host) is a device pointer; d_work 256-byte aligned, points 8-byte aligned.
 * Enqueues the reduction and the solve on `stream`.  d_H 9 floats, d_info APAP_MODEL_INFO doubles; d_status (may be NULL):
 * the status bits are OR-ed into it.  An argument error returns at once and enqueues nothing. */
int apap_model_solve_device(apap_ctx *ctx, const float *d_pts_c, const float *d_pts_o, const float *d_weights, int n,
                            const double *params, float *d_H, double *d_info, int *d_status, void *d_work, size_t work_bytes,
                            void *stream);
/* The EM loop of spectral_method() (:188-241) on one pair: em_steps rounds of
 *     calculate_M (apap_spectral_*, Hg = the previous round's H_pred; the first round takes mask_in)
 *     model_solve(ransac_mask)  (weights floor 1e-3, swap; model_params' FLOOR and SWAP are overridden)
 * on one stream (the resident form without any host synchronisation).  Outputs per round k (k = 0 .. em_steps-1): H_out[9 k], info_out[APAP_MODEL_INFO k],
 * segment_out[n k], ransac_mask_out[n k], original_mask_out[n k], spec_info_out[APAP_SPECTRAL_INFO k].  mask_in: the first
 * round's initial mask (what match_RANSAC returned), n float32.  Host-buffer call: with 1 <= em_steps <= 64, H_out and
 * info_out are set to NaN before anything else; an argument error returns APAP_ERR_INVALID_ARG and writes nothing more.
 * Once the kernels ran every output holds its round's results and the call returns the error of the first round whose
 * M-step reported APAP_STATUS_MODEL_DEGENERATE or APAP_STATUS_SINGULAR (as apap_model_solve).  Like apap_spectral_weights it
 * waits for each spectral restart cycle and stops at convergence (the resident form enqueues every cycle; same results). */
int apap_spectral_em(apap_ctx *ctx, const float *src, const float *dst, const float *c_feats, const float *o_feats, int n,
                     const double *F, const double *spec_params, const double *model_params, int em_steps, const float *mask_in,
                     float *H_out, double *info_out, double *segment_out, float *ransac_mask_out, float *original_mask_out,
                     double *spec_info_out, int device);
/* Resident form of apap_spectral_em: device pointers but the two parameter blocks; d_work of at least
 * apap_spectral_workspace_bytes(n) + apap_model_workspace_bytes(n) bytes, 256-byte aligned.  d_status (may be NULL) collects
 * every round's status bits.  Enqueues every round, every spectral restart cycle included (those after convergence return at
 * once but each costs its launch), and does not wait. */
int apap_spectral_em_device(apap_ctx *ctx, const float *d_src, const float *d_dst, const float *d_c_feats, const float *d_o_feats,
                            int n, const double *d_F, const double *spec_params, const double *model_params, int em_steps,
                            const float *d_mask_in, float *d_H, double *d_info, double *d_segment, float *d_ransac_mask,
                            float *d_original_mask, double *d_spec_info, int *d_status, void *d_work, size_t work_bytes,
                            void *stream);

/* The EM loop for a BATCH of independent problems on one stream: a problem is a pair, a set of spectral options and a set
 * of model options.  The problems advance in lockstep; the number of kernel launches does not depend on n_problems (a batch
 * whose pairs fall into several rows-per-block classes of the matrix-vector product takes one such launch per class, at most
 * 4).  Every output of every problem equals, byte for byte, what apap_spectral_em_device returns for that problem alone.
 *   src, dst, c_feats, o_feats, mask_in   the pairs concatenated: pair p holds matches pair_offset[p] .. pair_offset[p + 1] - 1
 *   F                 n_pairs x 9
 *   pair_offset       HOST, n_pairs + 1 entries, strictly increasing
 *   pair_of           HOST, n_problems entries: the pair of each problem (the problems of one pair read the same arrays)
 *   spec_params       HOST, n_problems x APAP_SPECTRAL_PARAMS; APAP_SPECTRAL_MAX_RESTARTS must be equal across the batch (the
 *                     cap fixes how many cycles are enqueued)
 *   model_params      HOST, n_problems x APAP_MODEL_PARAMS (FLOOR and SWAP overridden as in apap_spectral_em_device); LMS and
 *                     SDP problems may be mixed
 * Outputs are problem-major and round-major inside a problem: H[(b em_steps + k) 9], info[(b em_steps + k) APAP_MODEL_INFO],
 * spec_info[(b em_steps + k) APAP_SPECTRAL_INFO]; the per-match outputs of problem b start at em_steps x (the matches of the
 * problems before b), round k at + k n.  status: n_problems words (may be NULL), each collecting its own problem's bits; the
 * device form ORs into them (zero them first), the host-buffer form writes them.  A degenerate, singular or unconverged
 * problem sets its own status word and info blocks only, and the call still returns APAP_OK: the batch entry points do not
 * turn a per-problem status into an error code.  Bad arguments (null pointers, counts below 1, pair_of out of range, offsets
 * not increasing, em_steps outside 1 .. 64, bad per-problem parameters, a short or misaligned workspace) are refused before
 * any device is touched.
 * The device form enqueues every restart cycle and does not wait; the host-buffer form waits after each cycle and stops
 * enqueuing a round's cycles once every problem reports convergence.  Both give the same bytes.  d_work: at least
 * apap_spectral_em_batch_workspace_bytes(...) bytes (0 for invalid arguments), 256-byte aligned. */
size_t apap_spectral_em_batch_workspace_bytes(const int *pair_offset, int n_pairs, const int *pair_of, int n_problems);
int apap_spectral_em_batch_device(apap_ctx *ctx, const float *d_src, const float *d_dst, const float *d_c_feats,
                                  const float *d_o_feats, const double *d_F, const float *d_mask_in, const int *pair_offset,
                                  int n_pairs, const int *pair_of, const double *spec_params, const double *model_params,
                                  int n_problems, int em_steps, float *d_H, double *d_info, double *d_segment, float *d_ransac_mask,
                                  float *d_original_mask, double *d_spec_info, int *d_status, void *d_work, size_t work_bytes,
                                  void *stream);
int apap_spectral_em_batch(apap_ctx *ctx, const float *src, const float *dst, const float *c_feats, const float *o_feats,
                           const double *F, const float *mask_in, const int *pair_offset, int n_pairs, const int *pair_of,
                           const double *spec_params, const double *model_params, int n_problems, int em_steps, float *H_out,
                           double *info_out, double *segment_out, float *ransac_mask_out, float *original_mask_out,
                           double *spec_info_out, int *status_out, int device);

/* ------------------------------------------------- robust moving DLT: the M-step's solve per mesh cell --- */
/* What the comment above the SVD of the reference's cell loop asks for (apap.py:155-157): every cell's plain weighted DLT
 * replaced by the M-step's robust solve (LMS or SDP, above), the cell's moving-DLT weights folded into the match weights.
 * For cell k with vertex v_k:
 *     W_k[i] = max(exp(-|v_k - pts_c[i]| / sigma^2), gamma)          float64: the weight of apap_local_weights_pts
 *     w_k[i] = float32(W_k[i]) * match_weights[i]                    one float32 multiply; float32(W_k[i]) without match_weights
 * and cell k's H (9 float32), info (APAP_MODEL_INFO doubles) and status word equal, byte for byte, what
 * apap_model_solve_device(pts_c, pts_o, w_k, n, params) gives for that cell alone, whatever other cells are in the call.
 * The cells x n weights are never stored.
 *   pts_c, pts_o     n x 2 float32; distances are measured to pts_c.  With APAP_MODEL_SWAP 0 a cell's H maps pts_c -> pts_o
 *                    (the direction of apap_local_homography's src -> dst)
 *   match_weights    n float32, may be NULL (none): typically the last round's ransac_mask of apap_spectral_em
 *   vertices         cells x 2 float64 (get_vertice)
 *   params           HOST, APAP_MODEL_PARAMS doubles; MODE, DU, DV, FLOOR, SWAP and MAX_ITER are honoured as given
 *   H                cells x 9 float32;  info (may be NULL) cells x APAP_MODEL_INFO doubles
 *   status           cells words (may be NULL): each collects its own cell's bits.  The device form ORs into them (zero them
 *                    first), the host-buffer form writes them
 * A degenerate (fewer than 4 selected matches, or rank-deficient), singular or unconverged cell sets only its own status
 * word, its NaN H and its info block; the call still returns APAP_OK.
 * Refused before any device is touched: null pointers, n outside 1 .. 2^26, cells outside 1 .. APAP_LOCAL_MODEL_MAX_CELLS, a bad
 * mode / swap / max_iter, du or dv negative or not finite, sigma not a finite number > 0, a NaN gamma, a short
 * (APAP_ERR_WORKSPACE) or misaligned workspace.
 * Workspace: one cell's scratch is O(n / 240) 15 x 15 factors (16.5 KB at n = 2000).  apap_local_model_workspace_bytes
 * returns the scratch of min(cells, APAP_LOCAL_MODEL_CHUNK) cells (0 for invalid arguments; a 256-byte multiple).  The
 * device form processes the cells in chunks of as many cells as the workspace it is GIVEN holds (at least one cell's scratch,
 * else APAP_ERR_WORKSPACE; at most 65535 per chunk): two kernel launches per chunk, whatever the number of cells in it.
 * Under APAP_OPT_PROFILE the reductions are counted in the APAP_PROF_ASSEMBLE slot and the solves in APAP_PROF_EIGEN.
 * The host-buffer form sets H_out (and info_out) to NaN and status_out to 0 before anything else. */
#define APAP_LOCAL_MODEL_CHUNK 4096
#define APAP_LOCAL_MODEL_MAX_CELLS (1 << 24)
size_t apap_local_model_workspace_bytes(int n, int cells);
int apap_local_model_solve_device(apap_ctx *ctx, const float *d_pts_c, const float *d_pts_o, const float *d_match_weights, int n,
                                  const double *d_vertices, int cells, double gamma, double sigma, const double *params,
                                  float *d_H, double *d_info, int *d_status, void *d_work, size_t work_bytes, void *stream);
int apap_local_model_solve(apap_ctx *ctx, const float *pts_c, const float *pts_o, const float *match_weights, int n,
                           const double *vertices, int cells, double gamma, double sigma, const double *params, float *H_out,
                           double *info_out, int *status_out, int device);

/* ------------------------------------------------- descriptor matching: exact nearest and second-nearest, L2 --- */
/* The exact answer that coarse_matching's cv.FlannBasedMatcher().match(feats_cp, feats_op) approximates (utils.py:142-151):
 * for every query row i of q (nq x APAP_MATCH_DIM float32) the train row of t (nt x APAP_MATCH_DIM float32) at the smallest
 *     d2(i, j) = sum_k (q[i, k] - t[j, k])^2      float32, difference form: a subtraction and an fmaf per term, k ascending
 * and the runner-up.  For integer-valued descriptors in 0 .. 255 (OpenCV's SIFT) d2 <= 8 323 200 < 2^24 is exact.
 *   idx     nq int32: the j of the smallest d2(i, j); among equal d2 the lowest j
 *   dist    nq float32: the correctly rounded float32 square root of that float32 d2 (DMatch.distance)
 *   idx2, dist2   the same over j != idx[i]; both may be NULL (nearest only)
 * A d2 that is NaN or infinite is never selected.  Where no train row can be selected (and for the runner-up when nt = 1)
 * the index is -1 and the distance +inf.  The outputs are a function of (q, t) alone: no floating-point atomics, the same
 * bytes from every entry point below, whatever the launch geometry and whatever else is in a batch.
 * Batch: the pairs are concatenated; pair p holds the query rows q_offset[p] .. q_offset[p + 1] - 1 and the train rows
 * t_offset[p] .. t_offset[p + 1] - 1 (both HOST arrays of n_pairs + 1 strictly increasing entries; the device arrays are
 * indexed by them as given, the host-buffer form reads and writes from q_offset[0] / t_offset[0] on).  The outputs are laid
 * out like the queries; a pair's indices count from its own first train row.  Two kernel launches, whatever n_pairs; every
 * pair's outputs equal, byte for byte, its own single call's (the single call is the batch of one).
 * Refused before any device is touched: null required pointers, nq or nt (per pair) outside 1 .. 2^24, n_pairs outside
 * 1 .. 65535, negative or not strictly increasing offsets, a short (APAP_ERR_WORKSPACE) or misaligned workspace (256 bytes;
 * q and t 16 bytes).  Without a GPU the host-buffer forms return APAP_ERR_NO_DEVICE: there is no CPU fallback.
 * The _device forms only enqueue on `stream` (an upload of n_pairs small descriptors and two kernels) and do not wait.
 * d_work: at least apap_match_workspace_bytes(nq, nt) / apap_match_batch_workspace_bytes(...) bytes (0 for invalid arguments;
 * a 256-byte multiple): one 16-byte partial per query and split of the train axis.
 * The tiling (for tests and sizing; no output depends on it): a block takes APAP_MATCH_QUERY_TILE queries, the train rows go
 * in chunks of APAP_MATCH_TRAIN_CHUNK, and the chunks are dealt to min(chunks, ceil(APAP_MATCH_WANT_BLOCKS / query tiles))
 * splits of equal length (the last may be shorter). */
#define APAP_MATCH_DIM 128            /* = APAP_SPECTRAL_DIM */
#define APAP_MATCH_QUERY_TILE 64
#define APAP_MATCH_TRAIN_CHUNK 128
#define APAP_MATCH_WANT_BLOCKS 4096
size_t apap_match_workspace_bytes(int nq, int nt);
int apap_match_descriptors(apap_ctx *ctx, const float *q, int nq, const float *t, int nt, int *idx, float *dist, int *idx2,
                           float *dist2, int device);
int apap_match_descriptors_device(apap_ctx *ctx, const float *d_q, int nq, const float *d_t, int nt, int *d_idx, float *d_dist,
                                  int *d_idx2, float *d_dist2, void *d_work, size_t work_bytes, void *stream);
size_t apap_match_batch_workspace_bytes(const int *q_offset, const int *t_offset, int n_pairs);
int apap_match_descriptors_batch(apap_ctx *ctx, const float *q, const float *t, const int *q_offset, const int *t_offset,
                                 int n_pairs, int *idx, float *dist, int *idx2, float *dist2, int device);
int apap_match_descriptors_batch_device(apap_ctx *ctx, const float *d_q, const float *d_t, const int *q_offset,
                                        const int *t_offset, int n_pairs, int *d_idx, float *d_dist, int *d_idx2, float *d_dist2,
                                        void *d_work, size_t work_bytes, void *stream);

/* ------------------------------------------------- guided descriptor matching: nearest and second-nearest under a gate --- */
/* What recompute_matching's docstring asks for (spectral_method.py:35-64): apap_match_descriptors' answer, searched for every
 * query only among the train rows that a geometric model allows - a homography within a radius, an epipolar line within a
 * distance, a local-homography grid (DESIGN.md "Guided matching"; operation by operation in tests/guided_match_spec.py).
 * Records: each keypoint of either side carries three float64, built by apap_guided_records[_device] from pts (n x 2
 * float32) and model (9 doubles, row-major; a DEVICE pointer in the _device form).  With X = (double)x, Y = (double)y, every
 * operation a single IEEE float64 operation in the order written:
 *   APAP_GUIDED_REC_POINT     (X, Y, 1); the model is ignored and may be NULL
 *   APAP_GUIDED_REC_PROJECT   u = (M0 X + M1 Y) + M2, v = (M3 X + M4 Y) + M5, s = (M6 X + M7 Y) + M8: (u / s, v / s, 1)
 *   APAP_GUIDED_REC_LINE      ((M0 X + M1 Y) + M2, (M3 X + M4 Y) + M5, (M6 X + M7 Y) + M8)
 * A NULL model is refused for the last two.  Non-finite coordinates and s = 0 are no errors: they give the record that IEEE
 * arithmetic gives.  n outside 1 .. 2^24 and an unknown `what` are refused.
 * Gate of a query record A and a train record B, under r2 (one double per pair; >= 0 or +inf, NaN and negative refused):
 *   APAP_GUIDED_POINT   dx = B0 - A0, dy = B1 - A1, g = dx dx + dy dy; the pair passes iff g < r2
 *   APAP_GUIDED_LINE    e = (A0 B0 + A1 B1) + A2, n = A0 A0 + A1 A1; the pair passes iff e e < r2 n
 * The test is strict (the reference's dist < em_radius) and a NaN anywhere fails it: r2 = 0 passes nothing, r2 = +inf passes
 * every pair of finite POINT records.
 * Match: d2(i, j) is apap_match_descriptors' float32 value, bit for bit.  Over the train rows j that pass query i's gate:
 *   idx, dist, idx2, dist2   as apap_match_descriptors': ordered by (d2, j), a NaN or infinite d2 never selected, dist the
 *                            correctly rounded float32 square root, an empty slot -1 / +inf; idx2, dist2 may be NULL
 *   count   nq int32, may be NULL: the train rows that pass the gate, whatever their d2
 *   ridx, rdist   nt int32 / float32, both NULL to skip: for every train row the best query under the same predicate and the
 *                 same d2, ordered by (d2, i) - what a mutual check needs, without a second call
 * The outputs are a function of the inputs alone: no nq x nt buffer, no floating-point atomics, the same bytes from every
 * entry point below, whatever the launch geometry and whatever else is in a batch.
 * Batch: as apap_match_descriptors_batch - HOST q_offset / t_offset of n_pairs + 1 entries, records and descriptors
 * concatenated, outputs laid out like the queries (ridx, rdist like the train rows), indices counted from the pair's own first
 * row; one kind per call, r2[p] per pair (a HOST array in every form).  The launches do not depend on n_pairs (an upload of
 * the pairs' table, a fill when ridx is asked for, two kernels); every pair's outputs equal its own single call's byte for
 * byte (the single call is the batch of one).
 * Refused before any device is touched: what apap_match_descriptors refuses, an unknown kind, a bad r2, ridx without rdist or
 * the converse.  Without a GPU the host-buffer forms return APAP_ERR_NO_DEVICE: there is no CPU fallback.  The _device forms
 * only enqueue on `stream` and do not wait.  d_work: at least apap_match_guided[_batch]_workspace_bytes (0 for invalid
 * arguments; a 256-byte multiple): the table, 8 bytes per train row, 24 bytes per query and split of its pair's train axis.
 * The tiling (for tests and sizing; no output depends on it): a block takes APAP_GUIDED_QUERY_TILE queries, one per lane; the
 * train records go in chunks of APAP_GUIDED_TRAIN_CHUNK, dealt to min(chunks, ceil(APAP_GUIDED_WANT_BLOCKS / query tiles))
 * splits of equal length (the last may be shorter); a wave sums its survivors' d2 whenever APAP_GUIDED_DRAIN of them wait. */
#define APAP_GUIDED_REC_POINT 0
#define APAP_GUIDED_REC_PROJECT 1
#define APAP_GUIDED_REC_LINE 2
#define APAP_GUIDED_POINT 0
#define APAP_GUIDED_LINE 1
#define APAP_GUIDED_QUERY_TILE 256
#define APAP_GUIDED_TRAIN_CHUNK 128
#define APAP_GUIDED_DRAIN 64
#define APAP_GUIDED_WANT_BLOCKS 1024
int apap_guided_records(apap_ctx *ctx, const float *pts, int n, const double *model, int what, double *rec_out, int device);
int apap_guided_records_device(apap_ctx *ctx, const float *d_pts, int n, const double *d_model, int what, double *d_rec_out,
                               void *stream);
size_t apap_match_guided_workspace_bytes(int nq, int nt);
int apap_match_guided(apap_ctx *ctx, const double *rec_q, const float *q, int nq, const double *rec_t, const float *t, int nt,
                      int kind, double r2, int *idx, float *dist, int *idx2, float *dist2, int *count, int *ridx, float *rdist,
                      int device);
int apap_match_guided_device(apap_ctx *ctx, const double *d_rec_q, const float *d_q, int nq, const double *d_rec_t, const float *d_t,
                             int nt, int kind, double r2, int *d_idx, float *d_dist, int *d_idx2, float *d_dist2, int *d_count,
                             int *d_ridx, float *d_rdist, void *d_work, size_t work_bytes, void *stream);
size_t apap_match_guided_batch_workspace_bytes(const int *q_offset, const int *t_offset, int n_pairs);
int apap_match_guided_batch(apap_ctx *ctx, const double *rec_q, const double *rec_t, const float *q, const float *t,
                            const int *q_offset, const int *t_offset, int n_pairs, int kind, const double *r2, int *idx, float *dist,
                            int *idx2, float *dist2, int *count, int *ridx, float *rdist, int device);
int apap_match_guided_batch_device(apap_ctx *ctx, const double *d_rec_q, const double *d_rec_t, const float *d_q, const float *d_t,
                                   const int *q_offset, const int *t_offset, int n_pairs, int kind, const double *r2, int *d_idx,
                                   float *d_dist, int *d_idx2, float *d_dist2, int *d_count, int *d_ridx, float *d_rdist,
                                   void *d_work, size_t work_bytes, void *stream);

/* ------------------------------------------------- descriptor extraction: SIFT at given keypoints --- */
/* What coarse_matching asks of OpenCV before it matches (utils.py:142-151): cv.SIFT.create().compute(img, [cv.KeyPoint(x, y, 1)
 * ...]), one 128-d descriptor per given keypoint (size 1, default angle, octave 0).  The definition - OpenCV 4.x's, restated
 * without OpenCV - is in DESIGN.md "Descriptor extraction" and, operation by operation, in tests/sift_spec.py:
 *   grey    (h, w) uint8 as it is; (h, w, 3) uint8 is BGR, grey = (3735 B + 19235 G + 9798 R + 16384) >> 15
 *   base    the float32 grey image under a separable APAP_SIFT_TAPS-tap Gaussian, sigma = sqrt(1.6^2 - 0.5^2), reflect-101,
 *           rows first; never materialised: a keypoint reads an APAP_SIFT_PATCH x APAP_SIFT_PATCH patch of the grey image
 *   pt      (rint(x), rint(y)), round half to even; APAP_SIFT_SAMPLES samples at the offsets |i|, |j| <= 3, one counts if
 *           0 < pt.y + i < h - 1 and 0 < pt.x + j < w - 1; gradient by central differences, magnitude x window weight,
 *           orientation (the library's own atan2, <= 2e-6 rad) against 361 degrees, trilinear spread over 4 x 4 x 8 bins
 *   out     clamp at 0.2 of the norm, scale to norm 512, round, saturate to 0 .. 255; float32 (n, APAP_SIFT_DIM): what SIFT
 *           returns and what apap_match_descriptors takes.  A keypoint without a valid sample is 128 zeros, never NaN.
 * Every operation is a single IEEE float32 operation in a fixed order (no fused multiply-add, no floating-point atomics): the
 * outputs are a function of the image bytes and the float32 coordinates alone - the same bytes from every entry point below,
 * whatever the launch geometry and whatever else is in a batch.
 *   apap_sift_window   host only: the APAP_SIFT_SAMPLES x APAP_SIFT_WINDOW_COLS float32 table of the samples, rows in the order
 *                      (i, j) ascending: rbin, cbin, window weight exp(-(c_rot^2 + r_rot^2) / 8), rbin - floor(rbin),
 *                      cbin - floor(cbin), floor(rbin), floor(cbin), 0 - evaluated in float64 and rounded
 *   apap_sift_taps     host only: the APAP_SIFT_TAPS float32 taps, likewise
 * Batch: n_images images of their own shapes (HOST arrays heights, widths, channels and a HOST array of the image pointers -
 * device pointers for the _device form); the keypoints (x, y) float32 concatenated, image m holds rows pt_offset[m] ..
 * pt_offset[m + 1] - 1 (a HOST array of n_images + 1 strictly increasing entries; the device arrays are indexed by them as
 * given, the host-buffer form reads and writes from pt_offset[0] on).  One small upload and one kernel launch, whatever
 * n_images; every image's rows equal, byte for byte, its own single call's (the single call is the batch of one).
 * Refused before any device is touched: null pointers, sides outside 7 .. 32768, channels other than 1 or 3, a count of
 * keypoints (per image) outside 1 .. 2^24, n_images outside 1 .. 65535, negative or not strictly increasing offsets, a
 * non-finite coordinate (host-buffer forms; the _device forms give such a keypoint 128 zeros), a short (APAP_ERR_WORKSPACE)
 * or misaligned workspace (256 bytes).  Without a GPU the host-buffer forms return APAP_ERR_NO_DEVICE: there is no CPU fallback.
 * The _device forms only enqueue on `stream` and do not wait.  d_work: at least apap_sift_workspace_bytes(n_images) bytes (0 for
 * an invalid count; a 256-byte multiple): 32 bytes per image.  A block of 64 x APAP_SIFT_BLOCK_KEYPOINTS threads takes
 * APAP_SIFT_BLOCK_KEYPOINTS consecutive keypoints of the concatenated list (for tests; no output depends on it). */
#define APAP_SIFT_DIM 128             /* = APAP_MATCH_DIM */
#define APAP_SIFT_SAMPLES 49
#define APAP_SIFT_TAPS 13
#define APAP_SIFT_PATCH 21
#define APAP_SIFT_WINDOW_COLS 8
#define APAP_SIFT_BLOCK_KEYPOINTS 4
int apap_sift_window(float *out);
int apap_sift_taps(float *out);
size_t apap_sift_workspace_bytes(int n_images);
int apap_sift_describe(apap_ctx *ctx, const uint8_t *img, int h, int w, int channels, const float *pts, int n, float *out, int device);
int apap_sift_describe_device(apap_ctx *ctx, const uint8_t *d_img, int h, int w, int channels, const float *d_pts, int n, float *d_out,
                              void *d_work, size_t work_bytes, void *stream);
int apap_sift_describe_batch(apap_ctx *ctx, const uint8_t *const *imgs, const int *heights, const int *widths, const int *channels,
                             int n_images, const float *pts, const int *pt_offset, float *out, int device);
int apap_sift_describe_batch_device(apap_ctx *ctx, const uint8_t *const *d_imgs, const int *heights, const int *widths,
                                    const int *channels, int n_images, const float *d_pts, const int *pt_offset, float *d_out,
                                    void *d_work, size_t work_bytes, void *stream);

/* ------------------------------------------------- keypoint orientation and the descriptor at an orientation --- */
/* What the entry points above leave out: the keypoint's dominant orientation and a descriptor taken in it, so that matching
 * survives an in-plane rotation of the second picture.  OpenCV 4.x's calcOrientationHist and calcSIFTDescriptor for a size-1,
 * octave-0 keypoint; the definition is in DESIGN.md "Keypoint orientation" and, operation by operation, in
 * tests/sift_orient_spec.py.  grey, base, pt, the gradients, atan2 and the rule that a sample counts only if 0 < r < h - 1 and
 * 0 < c < w - 1 are those of apap_sift_describe.
 *   angle   the 25 samples |i|, |j| <= 2 vote with weight exp(-(i^2 + j^2) / (2 0.75^2)) x magnitude for bin rint(ang / 10) of
 *           36; OpenCV's circular 1 4 6 4 1 smoothing; the FIRST largest bin, refined by the parabola through its neighbours;
 *           angle = 360 - 10 bin in [0, 360): cv.KeyPoint.angle.  Only the dominant peak is used (OpenCV adds a keypoint for
 *           every peak of 0.8 of it): row k stays keypoint k.  A keypoint without a valid sample, or a flat patch, has angle 0.
 *   out     ori = 360 - angle; the 121 samples |i|, |j| <= 5, rotated by ori (the library's own sin and cos, <= 2.1e-7) into
 *           the 4 x 4 x 8 bins, weight exp(-(i^2 + j^2) / 18); then as apap_sift_describe.  APAP_SIFT_DIM float32 a keypoint.
 * Single IEEE float32 operations in a fixed order: the same bytes from every entry point.
 *   apap_sift_orient*              angles out (one float32 a keypoint)
 *   apap_sift_describe_oriented*   angles non-null: the descriptors at those angles, each in [0, 360], and angles_out must be
 *                                  null; angles null: orientation and descriptor in one pass (the patch read and blurred once),
 *                                  the angles written to angles_out, which must not be null then
 *   apap_sift_orient_window        host only: the APAP_SIFT_ORIENT_SAMPLES float32 weights of the orientation samples, (i, j)
 *   apap_sift_descr_window         ascending; the APAP_SIFT_DESCR_SAMPLES weights of the descriptor samples, likewise
 * Batches, pt_offset, the counts, channels, alignments and the workspace (apap_sift_orient_workspace_bytes) are those of
 * apap_sift_describe_batch; angles are addressed like keypoints (row pt_offset[m] + k).  Sides are 13 .. 32768: a keypoint reads
 * an APAP_SIFT_ORIENT_PATCH x APAP_SIFT_ORIENT_PATCH patch of the grey image under one reflection.  The host-buffer forms refuse a
 * non-finite coordinate and an angle that is not in [0, 360] before any device is touched; the _device forms give such a
 * keypoint a zero row, and angle 0 from the orientation. */
#define APAP_SIFT_ORIENT_SAMPLES 25
#define APAP_SIFT_DESCR_SAMPLES 121
#define APAP_SIFT_ORIENT_PATCH 25
int apap_sift_orient_window(float *out);
int apap_sift_descr_window(float *out);
size_t apap_sift_orient_workspace_bytes(int n_images);
int apap_sift_orient(apap_ctx *ctx, const uint8_t *img, int h, int w, int channels, const float *pts, int n, float *angles, int device);
int apap_sift_orient_device(apap_ctx *ctx, const uint8_t *d_img, int h, int w, int channels, const float *d_pts, int n, float *d_angles,
                            void *d_work, size_t work_bytes, void *stream);
int apap_sift_orient_batch(apap_ctx *ctx, const uint8_t *const *imgs, const int *heights, const int *widths, const int *channels,
                           int n_images, const float *pts, const int *pt_offset, float *angles, int device);
int apap_sift_orient_batch_device(apap_ctx *ctx, const uint8_t *const *d_imgs, const int *heights, const int *widths, const int *channels,
                                  int n_images, const float *d_pts, const int *pt_offset, float *d_angles, void *d_work, size_t work_bytes,
                                  void *stream);
int apap_sift_describe_oriented(apap_ctx *ctx, const uint8_t *img, int h, int w, int channels, const float *pts, int n,
                                const float *angles, float *angles_out, float *out, int device);
int apap_sift_describe_oriented_device(apap_ctx *ctx, const uint8_t *d_img, int h, int w, int channels, const float *d_pts, int n,
                                       const float *d_angles, float *d_angles_out, float *d_out, void *d_work, size_t work_bytes,
                                       void *stream);
int apap_sift_describe_oriented_batch(apap_ctx *ctx, const uint8_t *const *imgs, const int *heights, const int *widths,
                                      const int *channels, int n_images, const float *pts, const int *pt_offset, const float *angles,
                                      float *angles_out, float *out, int device);
int apap_sift_describe_oriented_batch_device(apap_ctx *ctx, const uint8_t *const *d_imgs, const int *heights, const int *widths,
                                             const int *channels, int n_images, const float *d_pts, const int *pt_offset,
                                             const float *d_angles, float *d_angles_out, float *d_out, void *d_work, size_t work_bytes,
                                             void *stream);

/* ------------------------------------------------- corner detection: exact integer Harris corners --- */
/* The keypoints that apap_sift_describe takes, from the image alone: integer pixel corners (the descriptor rounds its
 * coordinates and reads the base level only, so nothing finer could be used).  Everything is integer arithmetic - no float,
 * no rounding; the definition is in DESIGN.md "Corner detection" and, in numpy int64, in tests/corner_spec.py:
 *   grey     (h, w) uint8 as it is; (h, w, 3) uint8 is BGR, grey = (3735 B + 19235 G + 9798 R + 16384) >> 15
 *   Ix, Iy   3 x 3 Sobel with reflect-101 indices: Ix = (g[y-1,x+1] + 2 g[y,x+1] + g[y+1,x+1]) - (g[y-1,x-1] + 2 g[y,x-1] +
 *            g[y+1,x-1]), Iy the same with rows and columns exchanged; -1020 .. 1020
 *   a, b, c  the unnormalised 3 x 3 box sums of Ix^2, Ix Iy, Iy^2, reflect-101 on the indices of the product images; < 2^24
 *   R        25 (a c - b^2) - (a + c)^2 in int64: 25 times Harris's det - k tr^2 at k = 0.04; |R| < 2.2e15
 *   corner   R > 0 and (R, -index), index = y w + x, lexicographically greater than that of every other pixel of the
 *            (2 radius + 1)^2 window inside the image: a plateau yields one corner, no two corners lie within `radius` of
 *            each other in both axes, so an image holds at most ceil(h / (radius + 1)) ceil(w / (radius + 1)) of them
 *   quality  with Rmax the largest corner response, a corner is kept if 1000 R >= quality_permille Rmax
 *   order    R descending, then index ascending; the first max_corners are returned
 *   pts      (max_corners, 2) float32 (x, y), integer-valued; response (max_corners) long long; *count int: rows from
 *            *count on are zero.  An image without corners (flat, or straight edges only) gives *count = 0: not an error.
 * The outputs are a function of the image bytes and (max_corners, radius, quality_permille) alone: the same bytes from every
 * entry point below, whatever the tile geometry, the order in which atomics append candidates and whatever else is in a batch.
 * Batch: n_images images of their own shapes (HOST arrays heights, widths, channels and a HOST array of the image pointers -
 * device pointers for the _device form), one set of parameters; image m writes rows m max_corners .. (m + 1) max_corners - 1
 * of pts and response, and count[m].  One small upload, one memset and two kernel launches, whatever n_images; every image's
 * outputs equal, byte for byte, its own single call's (the single call is the batch of one).
 * Refused before any device is touched: null pointers, sides outside 7 .. 32768, channels other than 1 or 3, radius outside
 * 1 .. APAP_CORNER_MAX_RADIUS, quality_permille outside 0 .. 1000, max_corners < 1, n_images outside 1 .. 65535, a short
 * (APAP_ERR_WORKSPACE) or misaligned workspace (256 bytes; pts and response 8).  Without a GPU the host-buffer forms return
 * APAP_ERR_NO_DEVICE: there is no CPU fallback.
 * The _device forms only enqueue on `stream` and do not wait.  d_work: at least apap_corner_workspace_bytes(...) bytes (0 for
 * invalid arguments; a 256-byte multiple): 48 + 16 bytes per image, and 16 bytes per possible corner (the bound above) twice,
 * the second time rounded up to a power of two.  A block takes a tile of APAP_CORNER_TILE_W x APAP_CORNER_TILE_H pixels (for
 * tests; no output depends on it). */
#define APAP_CORNER_TILE_W 64
#define APAP_CORNER_TILE_H 32
#define APAP_CORNER_MAX_RADIUS 16
size_t apap_corner_workspace_bytes(const int *heights, const int *widths, int n_images, int radius);
int apap_corner_detect(apap_ctx *ctx, const uint8_t *img, int h, int w, int channels, int max_corners, int radius,
                       int quality_permille, float *pts, long long *response, int *count, int device);
int apap_corner_detect_device(apap_ctx *ctx, const uint8_t *d_img, int h, int w, int channels, int max_corners, int radius,
                              int quality_permille, float *d_pts, long long *d_response, int *d_count, void *d_work, size_t work_bytes,
                              void *stream);
int apap_corner_detect_batch(apap_ctx *ctx, const uint8_t *const *imgs, const int *heights, const int *widths, const int *channels,
                             int n_images, int max_corners, int radius, int quality_permille, float *pts, long long *response,
                             int *count, int device);
int apap_corner_detect_batch_device(apap_ctx *ctx, const uint8_t *const *d_imgs, const int *heights, const int *widths,
                                    const int *channels, int n_images, int max_corners, int radius, int quality_permille,
                                    float *d_pts, long long *d_response, int *d_count, void *d_work, size_t work_bytes, void *stream);

/* ------------------------------------------------- image pyramid: grey levels at scales 2^-k and (3/4) 2^-k --- */
/* What lets detection and matching survive a change of scale: the corner detector and the descriptor run on every level as
 * on any other image, and the pack brings the levels' corners back into the base picture's frame.  Everything is integer
 * arithmetic; the definition is in DESIGN.md "Image pyramid and scale" and, in numpy int64, in tests/pyramid_spec.py:
 *   grey     level 0: (h, w) uint8 as it is; (h, w, 3) uint8 is BGR, grey = (3735 B + 19235 G + 9798 R + 16384) >> 15
 *   H(g)     shape ((h + 1) >> 1, (w + 1) >> 1); H(g)[y, x] = (sum_{i,j = -2..2} b_i b_j g[r(2y + i, h), r(2x + j, w)] + 128) >> 8,
 *            b = (1, 4, 6, 4, 1), r = reflect-101; one rounding at the end
 *   Q(g)     shape ((3h) >> 2, (3w) >> 2); per axis output 3k + r reads sources 4k + r and 4k + r + 1 with weights (5, 1),
 *            (3, 3), (1, 5) for r = 0, 1, 2 - linear interpolation at 4x/3 + 1/6; Q(g)[y, x] = (sum of wy wx g + 18) / 36
 *   levels   half_steps != 0: level 2k = H^k(level 0), scale 2^-k; level 2k + 1 = H^k(Q(level 0)), scale (3/4) 2^-k.
 *            half_steps = 0: level k = H^k(level 0).  The levels stop before the first with a side under
 *            APAP_PYRAMID_MIN_SIDE: apap_pyramid_layout returns how many there are, 1 .. n_levels
 *   scale    scale_num[l] / 2^scale_shift[l]: 1 / 2^k, or 3 / 2^(k + 2)
 *   base     the base-frame coordinate of level pixel x: x 2^k, or (2^(k + 3) x + 1) / 6 as one float64 division of the exact
 *            integer, rounded to float32; the same for y
 *   caps     the corner budget of level l at max_corners: min(max_corners, max(16, max_corners >> 2k)), or on a 3/4 level
 *            min(max_corners, max(16, (9 max_corners) >> (2k + 4))): apap_pyramid_level_caps, caps[n_levels]
 * apap_pyramid_layout (host only): heights, widths, scale_num, scale_shift [n_levels] and offsets [n_levels + 1] (any may be
 * NULL): level l lies at byte offsets[l] of the picture's level buffer, a 256-byte multiple, row-major uint8; offsets[count]
 * is the buffer's size.  Returns 0 for invalid arguments.  Level 0 is always written, for a grey picture too.
 * Batch: n_images pictures of their own shapes and channels, one n_levels and half_steps; their level buffers lie back to
 * back in `levels` in the order of the pictures (each a 256-byte multiple).  One upload and 1 + ceil((n_levels - 1) / 2)
 * launches at most, whatever n_images; a picture's levels equal its own single call's byte for byte.  Bytes of the buffer
 * outside the levels are not written.
 * apap_pyramid_keypoints: the pack.  Input: the batched detector's slabs over n_level_images level images (d_slab_pts
 * (n_level_images, slab_rows, 2), d_slab_response (n_level_images, slab_rows)) and, per level image, HOST counts (0 ..
 * slab_rows: the detector's count clamped to the level's cap), scale_num, scale_shift and level_index.  Output: the first
 * counts[m] rows of every level image concatenated - pts (N, 2) float32 in the base frame, level_pts (N, 2) float32 as the
 * detector wrote them (what the descriptor reads on the level image), level (N) int = level_index[m], response (N) long
 * long - and HOST level_offset[n_level_images + 1].  One upload and one launch; none when N = 0.
 * Refused before any device is touched: null pointers, sides outside APAP_PYRAMID_MIN_SIDE .. 32768, channels other than 1
 * or 3, n_levels outside 1 .. APAP_PYRAMID_MAX_LEVELS, n_images (n_level_images) outside 1 .. 65535, a count outside 0 ..
 * slab_rows, a short (APAP_ERR_WORKSPACE) or misaligned workspace or level buffer (256 bytes).  Without a GPU the host-buffer
 * forms return APAP_ERR_NO_DEVICE.  The _device forms only enqueue on `stream` and do not wait.  A block takes a source tile
 * of APAP_PYRAMID_TILE_W x APAP_PYRAMID_TILE_H pixels (for tests; no output depends on it). */
#define APAP_PYRAMID_MAX_LEVELS 16
#define APAP_PYRAMID_MIN_SIDE 32
#define APAP_PYRAMID_TILE_W 64
#define APAP_PYRAMID_TILE_H 32
int apap_pyramid_layout(int h, int w, int n_levels, int half_steps, int *heights, int *widths, long long *offsets, int *scale_num,
                        int *scale_shift);
int apap_pyramid_level_caps(int max_corners, int n_levels, int half_steps, int *caps);
size_t apap_pyramid_workspace_bytes(int n_images, int n_levels);
int apap_pyramid_build(apap_ctx *ctx, const uint8_t *img, int h, int w, int channels, int n_levels, int half_steps, uint8_t *levels,
                       int device);
int apap_pyramid_build_device(apap_ctx *ctx, const uint8_t *d_img, int h, int w, int channels, int n_levels, int half_steps,
                              uint8_t *d_levels, size_t levels_bytes, void *d_work, size_t work_bytes, void *stream);
int apap_pyramid_build_batch(apap_ctx *ctx, const uint8_t *const *imgs, const int *heights, const int *widths, const int *channels,
                             int n_images, int n_levels, int half_steps, uint8_t *levels, int device);
int apap_pyramid_build_batch_device(apap_ctx *ctx, const uint8_t *const *d_imgs, const int *heights, const int *widths,
                                    const int *channels, int n_images, int n_levels, int half_steps, uint8_t *d_levels,
                                    size_t levels_bytes, void *d_work, size_t work_bytes, void *stream);
size_t apap_pyramid_keypoints_workspace_bytes(int n_level_images);
int apap_pyramid_keypoints(apap_ctx *ctx, const float *slab_pts, const long long *slab_response, int slab_rows, const int *counts,
                           const int *scale_num, const int *scale_shift, const int *level_index, int n_level_images, float *pts,
                           float *level_pts, int *level, long long *response, int *level_offset, int device);
int apap_pyramid_keypoints_device(apap_ctx *ctx, const float *d_slab_pts, const long long *d_slab_response, int slab_rows,
                                  const int *counts, const int *scale_num, const int *scale_shift, const int *level_index,
                                  int n_level_images, float *d_pts, float *d_level_pts, int *d_level, long long *d_response,
                                  int *level_offset, void *d_work, size_t work_bytes, void *stream);

/* ------------------------------------------------- global warp and blend: image_warping of utils.py:93-127 --- */
/* The output stage of spectral_method.py -s (:226-232): img2warp (h2 x w2 x 3 uint8) goes through one 3 x 3 homography onto
 * a canvas that bounds it and img_base (h1 x w1 x 3 uint8), and the base picture is pasted or mean-blended onto it.  The
 * definition - OpenCV 4.x's fixed-point INTER_LINEAR / BORDER_CONSTANT(0) warpPerspective in its exact-integer form, restated
 * without OpenCV - is in DESIGN.md "Global warp and blend" and, in numpy int64 / float64, in tests/image_warp_spec.py:
 *   bounds   apap_image_warp_bounds (host only, no device): the corners (0,0), (0,h2), (w2,h2), (w2,0) through H (9 doubles,
 *            row-major) as cv.perspectiveTransform does - w = H6 x + H7 y + H8 in fp64, w = w ? 1 / w : 0, each coordinate
 *            (Hk0 x + Hk1 y + Hk2) w rounded to float32 - joined with the base picture's corners; out = xmin, ymin, xmax, ymax
 *            with min = trunc(float32(min - 0.5f)), max = trunc(float32(max + 0.5f)) (utils.py:105-106).  The canvas is
 *            (xmax - xmin) x (ymax - ymin), the base picture sits at (-xmin, -ymin) and always fits.  A non-finite corner, one
 *            beyond int32 or a canvas side outside 1 .. APAP_IMAGE_WARP_MAX_SIDE: APAP_ERR_INVALID_ARG
 *   M        9 doubles, row-major: canvas <- source, the reference's Ht.dot(H) (utils.py:108-114), formed by the caller
 *   warp     Minv = cofactors(M) / det3(M) in fp64 (cv::invert's closed form); per canvas pixel (x, y): X0 = Minv0 x + Minv1 y
 *            + Minv2 (left to right, no fused multiply-add), Y0, W0 likewise; W = W0 ? 32 / W0 : 0; X = rint(min(max(X0 W,
 *            -2^31), 2^31 - 1)) (half to even; a NaN takes -2^31), Y likewise; sx = clamp(X >> 5, -32768, 32767), ax = X & 31;
 *            per channel out = ((32-ax)(32-ay) p00 + ax (32-ay) p01 + (32-ax) ay p10 + ax ay p11 + 512) >> 10 over the taps
 *            src[sy, sx], src[sy, sx+1], src[sy+1, sx], src[sy+1, sx+1], a tap outside the source being 0
 *   blend    direct_blend = 1: the base picture overwrites the canvas at (off_x, off_y).  0: inside that rectangle
 *            out = (base + warped) >> 1 per channel where any channel of the warped pixel is non-zero, else base
 *   out      canvas_h x canvas_w x 3 uint8, rows contiguous
 * One fused kernel launch over the canvas: no intermediate canvas, no atomics.  The outputs are a function of the picture
 * bytes, M and the geometry alone: the same bytes from every entry point below, whatever else is in a batch.
 * Batch: n_problems problems in the same single launch, each with its own pictures (HOST arrays of pointers - device pointers
 * for the _device form; problems may share pictures), shapes, M (n_problems x 9), canvas size, offsets and blend mode (HOST
 * arrays); problem p writes its canvas at out + out_offset[p] bytes (a HOST array; the canvases must not overlap).  One small
 * upload and one kernel launch, whatever n_problems; every problem's canvas equals, byte for byte, its own single call's
 * (the single call is the batch of one).
 * Refused before any device is touched: null pointers, picture or canvas sides outside 1 .. APAP_IMAGE_WARP_MAX_SIDE, a base
 * picture that does not fit the canvas at the offsets (negative offsets included), direct_blend other than 0 or 1, a
 * non-finite M, det3(M) = 0 or an inverse that is not finite, n_problems outside 1 .. APAP_IMAGE_WARP_MAX_PROBLEMS, negative
 * or overlapping output offsets, a short (APAP_ERR_WORKSPACE) or misaligned workspace (256 bytes).  Without a GPU the
 * host-buffer forms return APAP_ERR_NO_DEVICE: there is no CPU fallback.
 * The _device forms only enqueue on `stream` and do not wait.  d_work: at least apap_image_warp_workspace_bytes(n_problems)
 * bytes (0 for an invalid count; a 256-byte multiple): 144 bytes per problem, no contract on its contents.  d_status (may be
 * NULL) is the status word of the other resident entry points; this kernel has no condition to report and never writes it. */
#define APAP_IMAGE_WARP_MAX_SIDE 32767
#define APAP_IMAGE_WARP_MAX_PROBLEMS 65535
int apap_image_warp_bounds(int h1, int w1, int h2, int w2, const double *H, int *out);
size_t apap_image_warp_workspace_bytes(int n_problems);
int apap_image_warp(apap_ctx *ctx, const uint8_t *base, int h1, int w1, const uint8_t *src, int h2, int w2, const double *M,
                    int canvas_w, int canvas_h, int off_x, int off_y, int direct_blend, uint8_t *out, int device);
int apap_image_warp_device(apap_ctx *ctx, const uint8_t *d_base, int h1, int w1, const uint8_t *d_src, int h2, int w2, const double *M,
                           int canvas_w, int canvas_h, int off_x, int off_y, int direct_blend, uint8_t *d_out, void *d_work,
                           size_t work_bytes, int *d_status, void *stream);
int apap_image_warp_batch(apap_ctx *ctx, const uint8_t *const *bases, const int *base_h, const int *base_w, const uint8_t *const *srcs,
                          const int *src_h, const int *src_w, const double *M, const int *canvas_w, const int *canvas_h,
                          const int *off_x, const int *off_y, const int *direct_blend, int n_problems, uint8_t *out,
                          const long long *out_offset, int device);
int apap_image_warp_batch_device(apap_ctx *ctx, const uint8_t *const *d_bases, const int *base_h, const int *base_w,
                                 const uint8_t *const *d_srcs, const int *src_h, const int *src_w, const double *M, const int *canvas_w,
                                 const int *canvas_h, const int *off_x, const int *off_y, const int *direct_blend, int n_problems,
                                 uint8_t *d_out, const long long *out_offset, void *d_work, size_t work_bytes, int *d_status, void *stream);

/* ------------------------------------------------- panorama: every view of a case on one canvas ------------------------ */
/* The centre picture (center_h x center_w x 3 uint8) and n_layers = 1 .. APAP_PANORAMA_MAX_LAYERS neighbours on one canvas,
 * in one fused pass (DESIGN.md "Panorama"; in numpy: tests/panorama_spec.py).  Layer k holds what apap_warp_device takes for
 * one pair - its picture (img_h[k] x img_w[k] x 3), its forward grid (mesh_rows[k] x mesh_cols[k] x 3 x 3 float32), its mesh
 * edges, its pair canvas (final_w[k], final_h[k]) and the offsets (off_x[k], off_y[k]) of the centre on it - and layers may
 * differ in all of them.  All per-layer arguments are HOST arrays of n_layers entries; the pointer arrays hold host pointers
 * in apap_panorama and device pointers in apap_panorama_device (layers may share a picture).
 *   canvas   OX = max off_x, OY = max off_y, W = OX + max(final_w - off_x), H = OY + max(final_h - off_y):
 *            apap_panorama_bounds (host only, no device) writes out = W, H, OX, OY
 *   layer    at canvas pixel (X, Y), with j = X - OX + off_x[k], i = Y - OY + off_y[k]: the pixel [i, j] of apap_local_warp of
 *            that layer where 0 <= j < final_w[k] and 0 <= i < final_h[k] - the same cell lookup, float64 chain, strict bounds
 *            test and truncation -, (0, 0, 0) elsewhere.  The centre's value is its pixel (X - OX, Y - OY) inside its
 *            rectangle, (0, 0, 0) outside
 *   mean     APAP_PANORAMA_MEAN: a value is present when any of its bytes is non-zero; each channel of the output is
 *            floor(sum of the present values / their number), 0 when none is present.  With one layer: apap_local_stitch
 *   paste    APAP_PANORAMA_PASTE: inside the centre's rectangle the centre, black pixels included; outside it the first
 *            present layer in the given order, or 0
 *   out      H x W x 3 uint8, rows contiguous
 *   status   d_status[n_layers] (zeroed by the caller): the set-up of layer k ORs APAP_STATUS_SINGULAR / APAP_STATUS_INDEX into
 *            d_status[k].  apap_panorama returns APAP_ERR_SINGULAR / APAP_ERR_INDEX for the first layer that reports one, with
 *            "layer k" in the message, and copies the n_layers words to its host array `status` (may be NULL) either way
 * n_layers set-up launches (the warp's own, one per layer) and one launch over the canvas.  The grids are not modified.
 * Refused before any device is touched (APAP_ERR_INVALID_ARG): null pointers, n_layers outside 1 .. APAP_PANORAMA_MAX_LAYERS,
 * an unknown mode, a centre that does not fit a pair canvas at its offsets (negative offsets included), a canvas of 2^31
 * pixels or more, a picture of fewer than 2 pixels, with a side of 2^24 or more or of 2 GiB or more, a mesh of 53 million
 * cells or more; a short (APAP_ERR_WORKSPACE) or misaligned workspace (256 bytes).  Without a GPU apap_panorama returns
 * APAP_ERR_NO_DEVICE: there is no CPU fallback.
 * apap_panorama_device only enqueues on `stream` and does not wait.  d_work: at least apap_panorama_workspace_bytes(...)
 * bytes (0 for invalid arguments; a 256-byte multiple), no contract on its contents.
 * apap_panorama_mean_of: the kernel's division, floor(sum / count) for count = 1 .. 17 and sum <= 255 count by one multiply
 * and shift (0 for count = 0), as a host function - so that it can be checked exhaustively without a device. */
#define APAP_PANORAMA_MAX_LAYERS 16
#define APAP_PANORAMA_MEAN 0
#define APAP_PANORAMA_PASTE 1
int apap_panorama_bounds(int center_h, int center_w, const int *final_w, const int *final_h, const int *off_x, const int *off_y,
                         int n_layers, int *out);
size_t apap_panorama_workspace_bytes(const int *mesh_rows, const int *mesh_cols, const int *final_w, const int *final_h, int n_layers);
unsigned apap_panorama_mean_of(unsigned sum, unsigned count);
int apap_panorama(apap_ctx *ctx, const uint8_t *center, int center_h, int center_w, const uint8_t *const *imgs, const int *img_h,
                  const int *img_w, const float *const *Hfwd, const int *mesh_rows, const int *mesh_cols, const double *const *mesh_w,
                  const int *n_w, const double *const *mesh_h, const int *n_h, const int *final_w, const int *final_h, const int *off_x,
                  const int *off_y, int n_layers, int mode, uint8_t *out, int *status, int device);
int apap_panorama_device(apap_ctx *ctx, const uint8_t *d_center, int center_h, int center_w, const uint8_t *const *d_imgs,
                         const int *img_h, const int *img_w, const float *const *d_Hfwd, const int *mesh_rows, const int *mesh_cols,
                         const double *const *d_mesh_w, const int *n_w, const double *const *d_mesh_h, const int *n_h,
                         const int *final_w, const int *final_h, const int *off_x, const int *off_y, int n_layers, int mode,
                         uint8_t *d_out, void *d_work, size_t work_bytes, int *d_status, void *stream);
/* The edge-ramp blend: the mean with a weight per sample, so that a picture fades out towards its own border instead of
 * ending in a step (in numpy: tests/panorama_ramp_spec.py).  Canvas, layer value, bounds test, truncation and presence are
 * the panorama's, unchanged; the argument lists are those of apap_panorama / apap_panorama_device with `ramp`, the ramp width
 * 1 .. APAP_PANORAMA_MAX_RAMP, in place of `mode`; the workspace is apap_panorama_workspace_bytes(...).
 *   weight   of the pixel (x, y) of an h x w picture: min(d, ramp) with d = min(x + 1, w - x, y + 1, h - y), at least 1
 *            (apap_panorama_ramp_weight, host only).  For layer k (x, y) is the SOURCE pixel the sample is gathered from, the
 *            truncated target coordinates; for the centre it is (X - OX, Y - OY).  A weight of the source, not a distance
 *            transform of the warped footprint: that keeps the blend in the one pass
 *   output   per channel floor(sum of weight x value / sum of weight) over the present samples, 0 where none is present; a
 *            black source pixel is absent whatever its weight.  ramp = 1 is APAP_PANORAMA_MEAN byte for byte
 * Refused like apap_panorama's arguments, before any device is touched: ramp outside 1 .. APAP_PANORAMA_MAX_RAMP.  The ramp is
 * not a mode of apap_panorama[_device]: those keep refusing every mode but the two above.
 * apap_panorama_ramp_quotients: the kernel's division, out[k] = floor(sum[k] / wsum[k]) for wsum = 1 .. 17 x 256 and
 * sum <= 255 wsum by one IEEE float32 division (0 for wsum = 0), as a host function over n values. */
#define APAP_PANORAMA_MAX_RAMP 256
int apap_panorama_ramp_weight(int x, int y, int w, int h, int ramp);
void apap_panorama_ramp_quotients(const unsigned *sum, const unsigned *wsum, int n, unsigned *out);
int apap_panorama_ramp(apap_ctx *ctx, const uint8_t *center, int center_h, int center_w, const uint8_t *const *imgs, const int *img_h,
                       const int *img_w, const float *const *Hfwd, const int *mesh_rows, const int *mesh_cols,
                       const double *const *mesh_w, const int *n_w, const double *const *mesh_h, const int *n_h, const int *final_w,
                       const int *final_h, const int *off_x, const int *off_y, int n_layers, int ramp, uint8_t *out, int *status,
                       int device);
int apap_panorama_ramp_device(apap_ctx *ctx, const uint8_t *d_center, int center_h, int center_w, const uint8_t *const *d_imgs,
                              const int *img_h, const int *img_w, const float *const *d_Hfwd, const int *mesh_rows,
                              const int *mesh_cols, const double *const *d_mesh_w, const int *n_w, const double *const *d_mesh_h,
                              const int *n_h, const int *final_w, const int *final_h, const int *off_x, const int *off_y, int n_layers,
                              int ramp, uint8_t *d_out, void *d_work, size_t work_bytes, int *d_status, void *stream);
/* Exposure gain compensation: one multiplicative gain per view, fitted to the views' overlaps (Brown & Lowe, IJCV 2007,
 * section 6), applied inside the fused pass (DESIGN.md "Panorama, gain compensation"; in numpy: tests/panorama_gain_spec.py).
 * View 0 is the centre, view k = 1 .. n_layers layer k - 1.  A view's sample at a canvas pixel, and whether it is present, are
 * the panorama's under the context's APAP_OPT_WARP_SAMPLING; I = r + g + b of the sample.
 *   statistics  over the canvas pixels with X % step == 0 and Y % step == 0 (step 1 .. APAP_PANORAMA_GAIN_MAX_STEP):
 *               N[a][b] the number of them at which a and b are both present, S[a][b] the sum of I_a over those; both
 *               (n_layers + 1)^2 uint64, row-major, the diagonal a view by itself.  Exact integers; the call zeroes the tables
 *   gains       the minimiser of 1/2 sum_{a != b} N_ab [(g_a m_ab - g_b m_ba)^2 / sigma_n^2 + (1 - g_a)^2 / sigma_g^2] with
 *               m_ab = S_ab / (3 N_ab) (the paper's sigma_n = 10, sigma_g = 0.1), by Cholesky in float64 in one fixed order
 *               of + - * / sqrt: the same bits from apap_panorama_gain_solve on the host and from the device.  A view that
 *               overlaps nothing has gain 1.  q = clamp(rint(4096 g), APAP_PANORAMA_GAIN_MIN_Q, APAP_PANORAMA_GAIN_MAX_Q).
 *               flag = 1 and every gain 1 if a pivot or a gain is not positive / finite (valid statistics cannot cause it)
 *   application a channel c of a sample of view v becomes min(255, (c q_v + 2048) >> 12) (apap_panorama_gain_apply, host
 *               only, over n bytes).  Presence, the ramp weight and paste's first present layer are decided on the UNGAINED
 *               sample; mean, paste and ramp then take the gained value.  q = 4096 everywhere is the ungained canvas
 * apap_panorama_gain[_device]: apap_panorama[_device]'s arguments with mode = APAP_PANORAMA_MEAN, APAP_PANORAMA_PASTE or
 * APAP_PANORAMA_RAMP, `ramp` (read for APAP_PANORAMA_RAMP only) and gain_q, n_layers + 1 HOST ints.
 * apap_panorama_gain_stats[_device]: the geometry arguments and `step`; N, S host arrays / d_N, d_S device arrays.
 * apap_panorama_auto_gain_device: statistics, the solve on the device and the gained blend, all enqueued on `stream`, no
 * wait; d_N, d_S, d_g (n_layers + 1 doubles), d_q (n_layers + 1 ints) and d_flag (one int) are written for the caller.
 * apap_panorama_auto_gain: the same on host buffers (N, S, g, q, flag receive the results; the solve runs on the host
 * between the two passes).  All device forms use the workspace of apap_panorama_workspace_bytes and nothing more.
 * Refused before any device is touched (APAP_ERR_INVALID_ARG): whatever apap_panorama refuses, step outside 1 .. 64, a q
 * outside 1024 .. 16383, sigmas that are not finite and positive, n_views outside 2 .. 17.  Without a GPU the compute entry
 * points return APAP_ERR_NO_DEVICE; apap_panorama_gain_solve and apap_panorama_gain_apply touch no device. */
#define APAP_PANORAMA_RAMP 2
#define APAP_PANORAMA_GAIN_MAX_STEP 64
#define APAP_PANORAMA_GAIN_MIN_Q 1024
#define APAP_PANORAMA_GAIN_MAX_Q 16383
int apap_panorama_gain_solve(const unsigned long long *N, const unsigned long long *S, int n_views, double sigma_n, double sigma_g,
                             double *g_out, int *q_out, int *flag_out);
int apap_panorama_gain_apply(const uint8_t *values, int n, int q, uint8_t *out);
int apap_panorama_gain_stats(apap_ctx *ctx, const uint8_t *center, int center_h, int center_w, const uint8_t *const *imgs,
                             const int *img_h, const int *img_w, const float *const *Hfwd, const int *mesh_rows, const int *mesh_cols,
                             const double *const *mesh_w, const int *n_w, const double *const *mesh_h, const int *n_h,
                             const int *final_w, const int *final_h, const int *off_x, const int *off_y, int n_layers, int step,
                             unsigned long long *N, unsigned long long *S, int *status, int device);
int apap_panorama_gain_stats_device(apap_ctx *ctx, const uint8_t *d_center, int center_h, int center_w, const uint8_t *const *d_imgs,
                                    const int *img_h, const int *img_w, const float *const *d_Hfwd, const int *mesh_rows,
                                    const int *mesh_cols, const double *const *d_mesh_w, const int *n_w,
                                    const double *const *d_mesh_h, const int *n_h, const int *final_w, const int *final_h,
                                    const int *off_x, const int *off_y, int n_layers, int step, unsigned long long *d_N,
                                    unsigned long long *d_S, void *d_work, size_t work_bytes, int *d_status, void *stream);
int apap_panorama_gain(apap_ctx *ctx, const uint8_t *center, int center_h, int center_w, const uint8_t *const *imgs, const int *img_h,
                       const int *img_w, const float *const *Hfwd, const int *mesh_rows, const int *mesh_cols,
                       const double *const *mesh_w, const int *n_w, const double *const *mesh_h, const int *n_h, const int *final_w,
                       const int *final_h, const int *off_x, const int *off_y, int n_layers, int mode, int ramp, const int *gain_q,
                       uint8_t *out, int *status, int device);
int apap_panorama_gain_device(apap_ctx *ctx, const uint8_t *d_center, int center_h, int center_w, const uint8_t *const *d_imgs,
                              const int *img_h, const int *img_w, const float *const *d_Hfwd, const int *mesh_rows,
                              const int *mesh_cols, const double *const *d_mesh_w, const int *n_w, const double *const *d_mesh_h,
                              const int *n_h, const int *final_w, const int *final_h, const int *off_x, const int *off_y, int n_layers,
                              int mode, int ramp, const int *gain_q, uint8_t *d_out, void *d_work, size_t work_bytes, int *d_status,
                              void *stream);
int apap_panorama_auto_gain(apap_ctx *ctx, const uint8_t *center, int center_h, int center_w, const uint8_t *const *imgs,
                            const int *img_h, const int *img_w, const float *const *Hfwd, const int *mesh_rows, const int *mesh_cols,
                            const double *const *mesh_w, const int *n_w, const double *const *mesh_h, const int *n_h,
                            const int *final_w, const int *final_h, const int *off_x, const int *off_y, int n_layers, int mode, int ramp,
                            int step, double sigma_n, double sigma_g, uint8_t *out, unsigned long long *N, unsigned long long *S,
                            double *g, int *q, int *flag, int *status, int device);
int apap_panorama_auto_gain_device(apap_ctx *ctx, const uint8_t *d_center, int center_h, int center_w, const uint8_t *const *d_imgs,
                                   const int *img_h, const int *img_w, const float *const *d_Hfwd, const int *mesh_rows,
                                   const int *mesh_cols, const double *const *d_mesh_w, const int *n_w, const double *const *d_mesh_h,
                                   const int *n_h, const int *final_w, const int *final_h, const int *off_x, const int *off_y,
                                   int n_layers, int mode, int ramp, int step, double sigma_n, double sigma_g, uint8_t *d_out,
                                   unsigned long long *d_N, unsigned long long *d_S, double *d_g, int *d_q, int *d_flag, void *d_work,
                                   size_t work_bytes, int *d_status, void *stream);

/* ------------------------------------------------- panorama: the two-band blend ---------------------------------------- */
/* Low spatial frequencies blended over the ramp's wide region, fine detail taken from ONE view, so that misregistration
 * cannot double it (Brown & Lowe, IJCV 2007, section 7, with two bands; DESIGN.md "Panorama, two-band blend"; in numpy, exact
 * integers: tests/panorama_band_spec.py).  Canvas, layer geometry, coordinates, the strict bounds test, truncation, presence
 * and sampling are the panorama's, unchanged; view 0 is the centre, view k layer k - 1.
 *   low-pass    of an h x w x 3 picture I with radius r = `band`, 0 .. APAP_PANORAMA_MAX_BAND, n = 2 r + 1:
 *               T[y][x][c] = the sum of I[clamp(y + dy, 0, h - 1)][clamp(x + dx, 0, w - 1)][c] over |dx|, |dy| <= r (the border
 *               is replicated), B = (T + (n^2 >> 1)) / n^2 rounded down; r = 0 gives B = I.  The blur lives in SOURCE space,
 *               once per picture - not on the warped canvas: the blend stays in the one canvas pass and needs no canvas-sized
 *               intermediate, the choice the ramp made for its weights.  apap_box_blur[_device] compute B alone.
 *   per pixel   for every view v: c_v, the panorama's sample of I_v (the pixel (ix, iy), or the fixed-point blend of four
 *               taps under APAP_SAMPLING_BILINEAR); b_v, the sample of B_v at the same place (the same pixel; the same taps
 *               and weights); D_v = min(x + 1, w - x, y + 1, h - y), the uncapped border distance of the source pixel
 *               (x, y) = (ix, iy), (X - OX, Y - OY) for the centre; w_v = min(D_v, ramp), the ramp blend's weight.
 *               v is present iff any byte of c_v is non-zero (b_v may be 0 for a present view).  With gain_q,
 *               c'_v = gain(c_v, q_v) and b'_v = gain(b_v, q_v), min(255, (c q + 2048) >> 12); without, c' = c and b' = b.
 *               L = floor(sum w_v b'_v / sum w_v) per channel over the present views; s = the present view with the largest
 *               D_v, the lowest index on ties; out = clip(L + c'_s - b'_s, 0, 255) per channel, (0, 0, 0) where no view is
 *               present.  Where one view is present the output is its (gained) sample whatever `band` is; band = 0 is
 *               apap_panorama_ramp byte for byte.
 * apap_panorama_band[_device]: apap_panorama_ramp[_device]'s arguments with `band` and gain_q (n_layers + 1 HOST ints, or NULL
 * for no gains) after `ramp`.  d_work: at least apap_panorama_band_workspace_bytes(...) bytes, 256-byte aligned:
 * apap_panorama_workspace_bytes(...) and, for band > 0, a 256-byte aligned slot per view for its low-pass picture; 0 for
 * invalid arguments.  Refused before any device is touched (APAP_ERR_INVALID_ARG): band outside 0 .. APAP_PANORAMA_MAX_BAND,
 * then whatever apap_panorama_ramp refuses, then a q of gain_q outside 1024 .. 16383.  Without a GPU the host-buffer forms
 * return APAP_ERR_NO_DEVICE; the device forms only enqueue on `stream`.  The band is not a mode of apap_panorama[_device] or of
 * the gain entry points.
 * apap_box_blur[_device]: out = B of the h x w x 3 picture (at least 1 pixel, below 2 GiB) for radius 0 .. 32; `out` must not
 * overlap the picture. */
#define APAP_PANORAMA_BAND 3
#define APAP_PANORAMA_MAX_BAND 32
int apap_box_blur(apap_ctx *ctx, const uint8_t *img, int h, int w, int radius, uint8_t *out, int device);
int apap_box_blur_device(apap_ctx *ctx, const uint8_t *d_img, int h, int w, int radius, uint8_t *d_out, void *stream);
size_t apap_panorama_band_workspace_bytes(int center_h, int center_w, const int *img_h, const int *img_w, const int *mesh_rows,
                                          const int *mesh_cols, const int *final_w, const int *final_h, int n_layers, int band);
int apap_panorama_band(apap_ctx *ctx, const uint8_t *center, int center_h, int center_w, const uint8_t *const *imgs, const int *img_h,
                       const int *img_w, const float *const *Hfwd, const int *mesh_rows, const int *mesh_cols,
                       const double *const *mesh_w, const int *n_w, const double *const *mesh_h, const int *n_h, const int *final_w,
                       const int *final_h, const int *off_x, const int *off_y, int n_layers, int ramp, int band, const int *gain_q,
                       uint8_t *out, int *status, int device);
int apap_panorama_band_device(apap_ctx *ctx, const uint8_t *d_center, int center_h, int center_w, const uint8_t *const *d_imgs,
                              const int *img_h, const int *img_w, const float *const *d_Hfwd, const int *mesh_rows,
                              const int *mesh_cols, const double *const *d_mesh_w, const int *n_w, const double *const *d_mesh_h,
                              const int *n_h, const int *final_w, const int *final_h, const int *off_x, const int *off_y, int n_layers,
                              int ramp, int band, const int *gain_q, uint8_t *d_out, void *d_work, size_t work_bytes, int *d_status,
                              void *stream);

#ifdef __cplusplus
}
#endif
#endif /* APAP_HIP_H */
