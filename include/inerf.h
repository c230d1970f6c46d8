/*
 * inerf.h - C ABI of libinerf.so: the MI355X (gfx950) implementation of IntrinsicNeRF's volumetric
 * render_rays hot path.
 *
 * The reference (zju3dv/IntrinsicNeRF) is pure Python on PyTorch and has no FFI of its own: the
 * "operator interface" of this path is the set of Python functions listed below.  Each entry point
 * of this header replaces the ATen op sequence of one of them and is what a ctypes / cffi / pybind
 * binding on the reference side would bind (INTEGRATION.md shows the ctypes stub).  Citations are
 * relative to the reference repository root.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 unless the parameter is marked [host];
 *   - the library never allocates device memory: outputs and scratch are caller-owned;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - return value: 0 = success, negative = INERF_E_* (never throws, never aborts);
 *   - thread-safe as long as concurrent calls use distinct streams and distinct output/workspace
 *     buffers; packed weights are read-only and may be shared.
 */
#ifndef INERF_H
#define INERF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INERF_VERSION_MAJOR 0
#define INERF_VERSION_MINOR 2
/* Bumped whenever a struct layout, an argument list or the packed-weight format of this header changes; bindings
 * compare it with inerf_abi_version() of the library they loaded (a stale .so then fails loudly, not silently). */
#define INERF_ABI_VERSION 40027

/* error codes */
#define INERF_OK              0
#define INERF_E_INVALID      -1   /* bad argument (null pointer, non-positive size, unknown variant ...) */
#define INERF_E_UNSUPPORTED  -2   /* configuration outside what the kernels implement (see each call)    */
#define INERF_E_WORKSPACE    -3   /* workspace pointer null or too small                                  */
#define INERF_E_HIP          -4   /* a HIP runtime call failed; inerf_last_hip_error() has the code       */

/* network variants */
#define INERF_VARIANT_OBJECT  0   /* object_level/run_nerf_helpers.py:247 NeRF (11 raw channels)          */
#define INERF_VARIANT_SSR     1   /* SSR/models/semantic_nerf.py:74 Semantic_NeRF (11 + C [+128] channels) */

/* render flags */
#define INERF_FLAG_WHITE_BKGD   1u   /* run_nerf.py:407-410 / model_utils.py:109-114                      */
#define INERF_FLAG_LINDISP      2u   /* run_nerf.py:467-468 (object-level only)                           */
#define INERF_FLAG_ENDPOINT     4u   /* SSR endpoint_feat: fine raw carries the 128-d views activation    */
#define INERF_FLAG_U_PER_RAY    8u   /* `u` is [N, n_importance] (random) instead of a shared [n_importance] */
/* inerf_encode_mlp*: run the colour heads only on sample points with positive density.  raw2outputs (run_nerf.py:359-412) forms
 * alpha = 1 - exp(-relu(sigma) * dist), so a point with sigma <= 0 has weight +0 and its colours enter every map as 0 * finite.
 * With the flag such a point's raw row is (0, 0, 0, sigma, 0, 0, 0, 0, 0, 0, 0); a point with !(sigma <= 0) - a NaN included - has
 * the row of the ungated call, bit for bit.  Honoured for the object-level network in INERF_PREC_F16X3 without the endpoint
 * feature, and only with a workspace (inerf_encode_mlp_workspace_bytes with the flag: the survivors' records, 1 028 B per point of a
 * sub-range, bounded by INERF_GATE_BYTES, default 2 GiB - with INERF_FLAG_GATE_PROBE no records: 12 B per point of a sub-range, see
 * there; inerf_encode_mlp, which has none, returns INERF_E_WORKSPACE); every other configuration runs
 * the ungated kernel.  inerf_render_rays sets it by itself for a pass whose raw tensor the caller does not receive
 * (raw_coarse / raw_fine NULL) and whose noise tensor is NULL (noise is added to sigma before the ReLU); INERF_GATE=0 in the
 * environment turns that off.  The maps are those of the ungated path (a zero-weight term may flip the sign of a zero sum).
 * ONE deviation: a gated point's heads are not evaluated, so they can neither raise INERF_STATUS_F16_RANGE nor turn a
 * zero-weight term into NaN - either would take a non-finite head activation on a point whose trunk is finite. */
#define INERF_FLAG_GATE_COLOUR 32u
/* With INERF_FLAG_GATE_COLOUR only (alone: INERF_E_INVALID): a one-product PROBE of the trunk in front of it.  The gate needs the
 * sign of sigma, not its value, of every point it culls: a probe kernel evaluates position encoding, the eight layers and the
 * density head on the f16 hi operands alone (a third of the matrix work), together with S = sum |w_alpha,k| h7_k + |b_alpha|, and
 * only its CANDIDATES - points with !(s < -kappa S), kappa = 2^-6, the power of two above eight times the largest |s - sigma| / S measured
 * (profiles/gate_probe_margin.txt); a NaN or an infinity is one - go through the exact trunk, as a list.  A
 * candidate's raw row is that of INERF_FLAG_GATE_COLOUR alone, bit for bit; a culled point's row is (0, 0, 0, s, 0, ...) with
 * the probe's s < 0 in place of the exact sigma <= 0, which reaches no map (raw2outputs applies a ReLU to it).
 * ONE deviation more: on this path the trunk's share of INERF_STATUS_F16_RANGE is decided on the probe's hi-only activations, for
 * every point, per tile of the probe (the same threshold, 7.5e3 unscaled, a factor 8.7 below f16's maximum; the probe's
 * activations are within 1e-3 of the exact ones, so the exact trunk cannot overflow on a point the probe did not flag).  The
 * exact trunk, whose tiles hold candidates of rays from anywhere in a sub-range, raises no flag of its own; the heads do, per point.
 * inerf_render_rays sets it wherever it sets the gate; INERF_PROBE=0 in the environment turns that off.
 * WORKSPACE.  The candidates take the exact trunk AND the heads in one kernel, so nothing is kept per point but the candidate list
 * (4 B) and the probe's (s, S) (8 B): inerf_encode_mlp_workspace_bytes, inerf_workspace_bytes and inerf_render_workspace_bytes with this
 * flag are smaller than with the gate alone by the records and the survivor list (1 028 B per point of a sub-range).  A sub-range holds
 * INERF_GATE_BYTES / 1 028 points as with the gate alone, or, the variable unset, up to 2^27 points (1.5 GiB).  A candidate with
 * sigma <= 0 has its heads evaluated and discarded: its row is the gate's, and it raises no flag behind the trunk.
 * INERF_GATE_FUSED=0 in the environment: the earlier sequence probe -> exact trunk of the list -> heads of the survivors' records, with
 * the gate's workspace and sub-ranges - the same rows, status words and margin state, bit for bit.
 *
 * THE MARGIN PER NETWORK.  kappa = 2^-6 is one constant for every network.  A caller that keeps a MARGIN STATE next to a packed blob -
 * INERF_GATE_STATE_BYTES of device memory, 8-byte aligned, zeroed when the blob is packed and again whenever it is packed anew - and
 * passes it (inerf_encode_mlp_margin `gate_state`, inerf_render_args.gate_state_coarse / gate_state_fine) gets that network's own:
 * the exact trunk computes sigma of every candidate, so it measures r = |s - sigma| / S on each of them for free, and a launch uses
 *   kappa = observed >= min_observed && isfinite(r_max) ? max(2^-9, 8 r_max) : 2^-6        (inerf_gate_kappa)
 * fixed at its start for all of its sub-ranges.  While the margin in use is safe every point with positive density is a candidate, so
 * the measured population is the population at risk; this is statistical evidence per network with the project's factor 8, not a
 * per-point bound.  There is no upper clamp: a network with 8 r_max > 2^-6 gets the larger margin.  Nothing
 * reads the state back, synchronises or allocates; a captured launch replays with whatever the state holds then.  One state serves
 * one stream at a time.  NULL: the constant, and the launches of a library without the state, bit for bit.  Words of the state
 * (written by the kernels alone): float r_max | float kappa_in_use | uint64 observed | uint32 launches | 3 reserved words. */
#define INERF_FLAG_GATE_PROBE 64u
#define INERF_GATE_STATE_BYTES 32

/* arithmetic of the MLP GEMMs (inerf_net_desc.precision) */
#define INERF_PREC_F32        0   /* v_mfma_f32_32x32x2_f32: exact fp32 products and accumulation             */
#define INERF_PREC_F16X3      1   /* every fp32 operand split into f16 hi + f16 (lo * 2^11); three f16 MFMA
                                     products hi*hi + 2^-11 (hi*lo + lo*hi), fp32 accumulation: 22-bit operands,
                                     fp32-level accuracy at the 16x faster f16 matrix pipe.  Activations above
                                     6e4 in magnitude cannot be represented: the kernel then raises
                                     INERF_STATUS_F16_RANGE in the caller's status word (re-run with F32).     */

/* bits of the device status word (inerf_encode_mlp / inerf_render_rays `status` argument) */
#define INERF_STATUS_F16_RANGE  1

#define INERF_BASE_CHANNELS   11   /* rgb3 sigma albedo3 shading residual3 (run_nerf_helpers.py:321)       */
#define INERF_ENDPOINT_DIM    128
#define INERF_RAY_FLOATS      11   /* o3 d3 near far viewdir3 (run_nerf.py:122-128, rays.py:251-255)       */
#define INERF_MAX_CLASSES     240  /* semantic classes supported by the packed layout                     */
/* Size limits of the per-ray stage kernels (one ray per 64-lane wavefront, its samples staged in LDS).  A shape outside
 * them is INERF_E_UNSUPPORTED - checked first: for an empty batch too, whatever the pointers, before anything is launched. */
#define INERF_MAX_SAMPLES     1024 /* inerf_composite[_backward]: samples per ray (16 chunks of 64)       */
#define INERF_MIN_COARSE      3    /* inerf_sample_fine: coarse depths per ray (two mid-point bins)       */
#define INERF_MAX_COARSE      256  /* inerf_sample_fine: coarse depths; inerf_sample_pdf: bins            */
#define INERF_MIN_BINS        2    /* inerf_sample_pdf: bin edges per ray (one weight)                    */
#define INERF_MAX_IMPORTANCE  512  /* inerf_sample_fine / inerf_sample_pdf: new samples per ray           */

const char* inerf_version(void);
int inerf_abi_version(void);          /* INERF_ABI_VERSION the library was built against */
const char* inerf_build_digest(void); /* sha256 (64 hex digits) of the sources, headers and compiler flags this library was built from */
int inerf_last_hip_error(void);

/* ---------------------------------------------------------------------------------------------
 * Network description and weight packing.
 * Replaces: the nn.Module parameter storage of NeRF (run_nerf_helpers.py:259-279) and Semantic_NeRF
 * (semantic_nerf.py:98-118) as seen by forward().  Fixed architecture D=8, W=256, skips=[4],
 * use_viewdirs=True - every shipped config (run_nerf.py:545-552, every SSR/configs yaml).
 * ------------------------------------------------------------------------------------------- */
typedef struct inerf_net_desc {
    int32_t variant;      /* INERF_VARIANT_*                                                       */
    int32_t n_classes;    /* SSR: semantic classes C (0 = semantic head absent); object: must be 0 */
    int32_t l_xyz;        /* multires       (0..10)  -> 3+6*l_xyz encoded position channels        */
    int32_t l_dir;        /* multires_views (0..4)   -> 3+6*l_dir encoded direction channels       */
    float   xyz_div;      /* encoder input divisor: 1 (object) / 10 (SSR, semantic_nerf.py:64)     */
    int32_t precision;    /* INERF_PREC_*: selects the packed format AND the MLP kernel            */
} inerf_net_desc;

/* Number of state-dict tensors the packer expects, and the canonical order/shape of tensor i:
 * pts_linears.{0..7}.{weight,bias}, views_linears.0, feature_linear, alpha_linear, then
 *   object: shading_linear (=residual head), albedo_linear1, albedo_linear2, test_linear1, test_linear2
 *   ssr   : [semantic_linear.0.0, semantic_linear.1,] residual_linear, albedo_linear1, albedo_linear2,
 *           shading_linear1, shading_linear2
 * (weight then bias for each).  inerf_tensor_info lets a binding verify a state dict; the returned
 * name pointer stays valid until the next inerf_tensor_info call on the same thread. */
int inerf_num_tensors(const inerf_net_desc* net);
int inerf_tensor_info(const inerf_net_desc* net, int index, const char** name /*[host] out*/,
                      int64_t* rows /*out*/, int64_t* cols /*out; 0 for a bias*/);

/* Size in floats of the packed blob for this network. */
int64_t inerf_packed_floats(const inerf_net_desc* net);

/* Pack the [host] fp32 state-dict tensors (row-major [out,in], canonical order above) into the
 * MFMA-fragment-ordered blob the kernels stream ([host] packed_out, inerf_packed_floats() floats).
 * The caller uploads the blob to the device once per weight update. */
int inerf_pack_weights(const inerf_net_desc* net, const float* const* tensors /*[host]*/, int n_tensors,
                       float* packed_out /*[host]*/, int64_t packed_capacity_floats);

/* ---------------------------------------------------------------------------------------------
 * Stage kernels (each is also a parity-test boundary).
 * ------------------------------------------------------------------------------------------- */

/* z_vals[N,S]: stratified depths.  Replaces run_nerf.py:464-486 / trainer.py:730-746.
 * rays[N,11]; t_vals[S] = linspace(0,1,S) supplied by the caller (so its rounding is the host
 * framework's); t_rand[N,S] or NULL (perturb == 0); lindisp via flags. */
int inerf_sample_coarse(const float* rays, const float* t_vals, const float* t_rand, int64_t n_rays, int n_samples,
                        uint32_t flags, float* z_out, void* stream);

/* raw[N,S,CH] = MLP(encode(o + d*z), encode(viewdir)).  Replaces run_network + NeRF.forward:
 * run_nerf.py:42-56 + run_nerf_helpers.py:195-243,284-321 / model_utils.py:19-35 +
 * semantic_nerf.py:14-65,123-181.  CH = 11 + n_classes (+128 if INERF_FLAG_ENDPOINT).
 * packed_weights: device copy of the inerf_pack_weights() blob.
 * status: optional device int32 the kernel ORs INERF_STATUS_* bits into (caller zeroes it). */
int inerf_encode_mlp(const inerf_net_desc* net, const float* packed_weights, const float* rays, const float* z_vals,
                     int64_t n_rays, int n_samples, uint32_t flags, float* raw_out, int32_t* status, void* stream);

/* The same with a caller-owned scratch buffer of inerf_encode_mlp_workspace_bytes() bytes (0 for most configurations).  With
 * it the INERF_PREC_F16X3 kernel of the SSR network splits the semantic hidden layer (semantic_nerf.py:110,150-152) over the
 * waves by channel and parks the per-wave partial logits in the scratch until the tile's activations are dead - the weights of
 * semantic_linear.0.0 are then streamed once per 64-point tile instead of four times.  Same results as inerf_encode_mlp up to
 * the summation order of the logits.  inerf_render_rays uses this form (its workspace includes the scratch). */
int64_t inerf_encode_mlp_workspace_bytes(const inerf_net_desc* net, int64_t n_rays, int n_samples, uint32_t flags);
int inerf_encode_mlp_ws(const inerf_net_desc* net, const float* packed_weights, const float* rays, const float* z_vals,
                        int64_t n_rays, int n_samples, uint32_t flags, float* raw_out, int32_t* status, void* workspace,
                        int64_t workspace_bytes, void* stream);
/* The same with ONE STATUS WORD PER `status_rays` RAYS: `status` then points at ceil(n_rays / status_rays) device words (caller
 * zeroes them) and word w collects the INERF_STATUS_* bits of rays [w * status_rays, (w + 1) * status_rays).  The front-ends render
 * an eval-mode frame as one launch whatever `chunk` the caller of batchify_rays (run_nerf.py:59-71, training_utils.py:5-17) asked
 * for and still learn WHICH of the caller's chunks left the f16 range - only that one is rendered again in exact fp32.
 * status_rays <= 0: one word, as inerf_encode_mlp_ws. */
int inerf_encode_mlp_chunked(const inerf_net_desc* net, const float* packed_weights, const float* rays, const float* z_vals,
                             int64_t n_rays, int n_samples, uint32_t flags, float* raw_out, int32_t* status, int64_t status_rays,
                             void* workspace, int64_t workspace_bytes, void* stream);
/* For tests of INERF_FLAG_GATE_PROBE: the same, and `probe_out` (device, [n_rays * n_samples, 2], or NULL) receives the probe's
 * (s, S) per point where the probe runs (it is left untouched where the flags do not select it). */
int inerf_encode_mlp_probed(const inerf_net_desc* net, const float* packed_weights, const float* rays, const float* z_vals,
                            int64_t n_rays, int n_samples, uint32_t flags, float* raw_out, int32_t* status, int64_t status_rays,
                            void* workspace, int64_t workspace_bytes, float* probe_out, void* stream);
/* The same with the probe's MARGIN STATE of this packed network (INERF_FLAG_GATE_PROBE above; device, INERF_GATE_STATE_BYTES, or NULL:
 * inerf_encode_mlp_probed).  Used where the probe runs, ignored elsewhere. */
int inerf_encode_mlp_margin(const inerf_net_desc* net, const float* packed_weights, const float* rays, const float* z_vals,
                            int64_t n_rays, int n_samples, uint32_t flags, float* raw_out, int32_t* status, int64_t status_rays,
                            void* workspace, int64_t workspace_bytes, float* probe_out, void* gate_state, void* stream);
/* [host] The margin a launch would use for a state that holds (r_max, observed), and the number of listed points a network has to be
 * measured on before its r_max is believed (INERF_PROBE_MIN_OBS in the environment overrides the built-in value). */
float inerf_gate_kappa(float r_max, int64_t observed, int64_t min_observed);
int64_t inerf_gate_min_observed(void);

/* ---------------------------------------------------------------------------------------------
 * Training: what autograd records for the network when the trainers call loss.backward()
 * (run_nerf.py:1018 through run_nerf_helpers.py:284-321; trainer.py:990 through
 * semantic_nerf.py:123-181).  Split-precision (INERF_PREC_F16X3) path only.
 *   forward : inerf_encode_mlp_train  = inerf_encode_mlp + every layer's output kept in `save`
 *   backward: inerf_mlp_backward_inputs: d raw -> pre-activation gradient dZ of every layer
 *             (the input-gradient chain, MFMA); the weight gradients are then plain GEMMs over the
 *             sample points, dW_l = dZ_l^T X_l, db_l = column sums of dZ_l, left to the caller's
 *             GEMM library.
 * `save` and `dz` are buffers of inerf_mlp_save_floats() 4-byte elements laid out [slot][point][width], every slot sized for
 * WHOLE 64-point tiles (64 * ceil(n_points / 64) points; inerf_mlp_save_slot() gives offset, width and format):
 *   slot 0 enc 64 | 1 dir 32 | 2..9 h0..h7 256 | 10 albedo|shading hidden 256 | 11 feature 256 |
 *   12 views hidden 128 | 13 semantic hidden 128 (SSR with classes, else width 0) |
 *   14 (dz only) head pre-activation gradients 8: albedo 3, shading 1, residual 3, sigma 1 | 15 unused (width 0).
 * Two slot formats:
 *   ROWS      a row-major fp32 [n_points, width] matrix.  save: 13; dz: 14.
 *   FRAGMENTS the operands of the 256-wide weight-gradient products dW = dZ^T X exactly as the matrix core consumes
 *             them: every value v is stored as f16 hi = f16(v') (towards zero; slots 0 and 1 of save, the encodings: to nearest,
 *             so there lo may have the other sign) and f16 lo = f16(v' - hi) in 1 KB fragments
 *             [32 channels x 16 points]; with kb = 16-point block of the tile (0..3), cb = 32-channel block:
 *               byte offset = (((tile * 4 + kb) * 8 + cb) * 2 + (0: hi, 1: lo)) * 1024 + lane * 16 + 2 * i      (i = 0..7)
 *               channel = 32 cb + (lane & 31),  point = 64 tile + 32 (kb >> 1) + (i & 3) + 8 ((i >> 2) + 2 (kb & 1)) + 4 (lane >> 5)
 *             (lane = channel, 8 k-values = 8 points: one 16-byte operand slot of v_mfma_f32_32x32x16_f16; the point order
 *             inside a block is the accumulator's register order).
 *             save, slots 2..11: v' = 8 v (the forward kernel's own operand halves); slots 12 (views hidden, 128 channels), 0 and 1
 *             (the encodings, 64 / 32 channels): the same with width / 32 = FOUR / TWO / ONE channel blocks per k-block instead of eight -
 *             byte offset = (((tile * 4 + kb) * (width / 32) + cb) * 2 + plane) * 1024 + ...
 *             dz, slots 2..11 and 12, 13 (the views / semantic hidden layers: 128 channels = FOUR blocks per k-block): v' = 8 v / s_p, s_p = the point's NORMALISER (the power of two above its largest head
 *             gradient; the chain works on normalised gradients, so these halves keep 22 bits whatever a point's gradient
 *             scale) - the normalisers are the first 64 * ceil(n_points / 64) floats of slot 0 of dz, and the weight-gradient
 *             kernels multiply them back in when they bring a fragment to the batch's max |dz|.
 *             Padding points of the last tile hold a copy of the last point (save) / zeros (dz).  Same 4 bytes per element as
 *             fp32; the producers write whole fragments and inerf_mlp_weight_gradient_frag moves them HBM -> LDS by DMA.
 * Behind the slots `save` carries the ReLU masks of h0..h7 as bits (16 384 bytes per 64-point tile, written by
 * inerf_encode_mlp_train and read by inerf_mlp_backward_inputs in place of the activations; layout private to the
 * two kernels) and 64 scalars: always pass a buffer that inerf_encode_mlp_train itself filled, of inerf_mlp_save_floats() floats.
 * The gradient w.r.t. the semantic logits is d_raw[..., 11:11+C] itself (no activation).
 * One kept evaluation is limited to 4 000 000 sample points (a slot is addressed through a 32-bit buffer descriptor):
 * inerf_encode_mlp_train, inerf_mlp_backward_inputs and inerf_mlp_backward return INERF_E_UNSUPPORTED beyond it; split a
 * larger batch into several evaluations and add the parameter gradients (the Python mirror does).
 * ------------------------------------------------------------------------------------------- */
#define INERF_SAVE_SLOTS 16
int64_t inerf_mlp_save_floats(const inerf_net_desc* net, int64_t n_points);
int inerf_mlp_save_slot(const inerf_net_desc* net, int slot, int64_t n_points, int64_t* offset_floats, int* width);
/* 1 when `slot` of the gradient buffer (gradient != 0) / the activation buffer is in FRAGMENT format, 0 for rows, negative: error */
int inerf_mlp_save_slot_is_fragment(int slot, int gradient);
int inerf_encode_mlp_train(const inerf_net_desc* net, const float* packed_weights, const float* rays, const float* z_vals,
                           int64_t n_rays, int n_samples, uint32_t flags, float* raw_out, float* save_out,
                           float* act_max /* optional device float the kernel max-es |activation| into (caller zeroes it): an upper bound of
                                             every |value| the slots of save decode to, at most 2^-10 of it + 2^-27 above the largest */,
                           int32_t* status, void* stream);

/* Transposed weights for the input-gradient chain, [host] -> [host] like inerf_pack_weights. */
int64_t inerf_bwd_packed_floats(const inerf_net_desc* net);
int inerf_pack_weights_bwd(const inerf_net_desc* net, const float* const* tensors /*[host]*/, int n_tensors,
                           float* packed_out /*[host]*/, int64_t packed_capacity_floats);

/* raw / d_raw: [n_points, CH] (CH as for inerf_encode_mlp with the same flags); save: from
 * inerf_encode_mlp_train on the same points; dz_out: every slot is written for every point. */
int inerf_mlp_backward_inputs(const inerf_net_desc* net, const float* packed_bwd, const float* raw, const float* d_raw,
                              const float* save, int64_t n_points, uint32_t flags, float* dz_out,
                              float* dz_max /* optional device float the kernel max-es |dz| into (caller zeroes it) */,
                              float* head_partial /* optional [inerf_mlp_backward_grid()][inerf_mlp_head_partial_floats()]:
                                 per-workgroup weight / bias gradients of the 1-4-row heads, to be summed by the caller:
                                 residual W [3][128] | albedo,shading outputs [4][256] (rows 0-2: columns 0..127 are
                                 albedo_linear2, row 3: columns 128..255 the shading output) | alpha W [256] |
                                 biases albedo 3, shading 1, residual 3, sigma 1 */,
                              int32_t* status, void* stream);
int inerf_mlp_head_partial_floats(void);
int inerf_mlp_backward_grid(int64_t n_points);

/* One weight gradient: workgroup g of inerf_wgrad_grid(n_points) writes sum over its sample points of G[p, m] * X[p, n]
 * (row-major [M, N]) at partial + g * partial_stride and, if bias_partial is given, its sums of G[p, m] ([M]) at
 * bias_partial + g * partial_stride; the caller adds the grid's tiles (deterministic, no atomics; several gradients can
 * share one [grid, partial_stride] buffer and one final sum).  G[P, ldg] / X[P, ldx]: row-major device
 * matrices (a slot of the gradient / activation buffers, or a 32-column-aligned part of one; pointers 16-byte
 * aligned, ld a multiple of 4); M in {128, 256}, N in {32, 64, 128, 256}.  ranges: device floats {gmax, xmax}, upper
 * bounds of |G| and |X| (e.g. the dz_max of inerf_mlp_backward_inputs; 7.5e3 for activations that passed the forward's
 * range check): the kernel scales the operands by the powers of two that bring those bounds into [2^13, 2^14).
 * The rows are read through 32-bit buffer descriptors: n_points * max(ldg, ldx) * 4 bytes (plus a 25 MB prefetch margin) must
 * stay below 4 GiB - INERF_E_UNSUPPORTED otherwise (4 000 000 points of a 256-wide slot fit). */
int inerf_wgrad_grid(int64_t n_points);
int inerf_mlp_weight_gradient(const float* G, int ldg, const float* X, int ldx, int64_t n_points, int M, int N,
                              const float* ranges, float* partial, float* bias_partial, int64_t partial_stride, void* stream);
/* The same with G a FRAGMENT slot of the gradient buffer (M = 256) - g_scale: the points' normalisers, slot 0 of that buffer,
 * see above - and X row-format: N in {64} (the encoding columns of pts_linears.0 / .5).  ranges as above (of the TRUE |dz|). */
int inerf_mlp_weight_gradient_gfrag(const void* G_frag, const float* g_scale, const float* X, int ldx, int64_t n_points, int N,
                                    const float* ranges, float* partial, float* bias_partial, int64_t partial_stride, void* stream);
/* G row-format (M = 128), X a FRAGMENT slot of the activation buffer (N = 256): views_linears.0's feature columns and the
 * semantic hidden layer.  ranges[0]: an upper bound of |G|. */
int inerf_mlp_weight_gradient_xfrag(const float* G, int ldg, const void* X_frag, int64_t n_points, int M,
                                    const float* ranges, float* partial, float* bias_partial, int64_t partial_stride, void* stream);
/* ... and with BOTH operands FRAGMENT slots (256 x 256: G of the gradient buffer, X of the activation buffer, same points):
 * a ring of LDS stages filled by LDS-DMA - bound by HBM bandwidth.  ranges[0]: an upper bound of the true |dz|.
 * _batch: n_jobs (<= INERF_WGRAD_MAX_BATCH) such products over the SAME points and normalisers in one launch of
 * inerf_wgrad_frag_grid(n_points, n_jobs) workgroups; g_rows[j] x x_cols[j] = 256 x 256, 256 x 64 (X the position encoding's
 * slot), 128 x 256 or 128 x 32 (G the views / semantic hidden layer's slot; X the view encoding's) - NULL: all 256.  Job j is split over
 * inerf_wgrad_frag_rows(n_points, n_jobs, g_rows, x_cols, j) of them (its share of the work), K-slice s
 * writing its [g_rows[j], x_cols[j]] tile at partial[j] + s * partial_stride (and its column sums of G at bias_partial[j] + s *
 * partial_stride where that entry is not NULL): ~n_jobs times fewer partial tiles to write and to sum than n_jobs single
 * launches.  The single form is the batch of one 256 x 256 product (inerf_wgrad_grid(n_points) slices). */
#define INERF_WGRAD_MAX_BATCH 16
int inerf_wgrad_frag_grid(int64_t n_points, int n_jobs);
int inerf_wgrad_frag_rows(int64_t n_points, int n_jobs, const int* g_rows /*[host] or NULL*/, const int* x_cols /*[host] or NULL*/, int job);
int inerf_mlp_weight_gradient_frag_batch(int n_jobs, const void* const* G_frag /*[host]*/, const float* g_scale, const void* const* X_frag /*[host]*/,
                                         const int* g_rows /*[host] or NULL*/, const int* x_cols /*[host] or NULL*/, const float* ranges,
                                         int64_t n_points, float* const* partial /*[host]*/,
                                         float* const* bias_partial /*[host] or NULL*/, int64_t partial_stride, void* stream);
int inerf_mlp_weight_gradient_frag(const void* G_frag, const float* g_scale, const void* X_frag, const float* ranges, int64_t n_points,
                                   float* partial, float* bias_partial, int64_t partial_stride, void* stream);

/* The network's whole backward pass in ONE call: the input-gradient chain, every weight-gradient product (split-K launches,
 * the workgroups' partial tiles side by side in the workspace) and one reduction that writes every sum into its place in
 * grads_out - the flat concatenation (inerf_param_floats() floats) of the reference's parameter tensors in
 * inerf_tensor_info() order, i.e. what autograd leaves in .grad of every nn.Linear after loss.backward()
 * (run_nerf.py:1018, trainer.py:990).  raw / d_raw [n_points, CH]; save: the buffer inerf_encode_mlp_train filled for these
 * points; act_max: the device float that call max-ed |activation| into.  workspace: inerf_mlp_backward_workspace_bytes()
 * bytes (the pre-activation gradients of every layer, 11 KB per point, live only there).  Asynchronous on `stream`,
 * deterministic (fixed summation order).  n_points == 0 zeroes grads_out. */
int64_t inerf_param_floats(const inerf_net_desc* net);
int64_t inerf_mlp_backward_workspace_bytes(const inerf_net_desc* net, int64_t n_points);
int inerf_mlp_backward(const inerf_net_desc* net, const float* packed_bwd, const float* raw, const float* d_raw, const float* save,
                       const float* act_max, int64_t n_points, uint32_t flags, float* grads_out, void* workspace,
                       int64_t workspace_bytes, int32_t* status, void* stream);

/* Where every element of a packed blob comes from, so that a caller can re-pack ON THE DEVICE after each
 * optimiser step (a gather, a per-group max for the power-of-two scales, an f16 hi/lo split) instead of moving the
 * weights through the host.  backward = 0: the INERF_PREC_F16X3 blob of inerf_pack_weights; 1: the blob of
 * inerf_pack_weights_bwd.  Per half-precision position of the blob (2 per float): half_src = 1 + index into the
 * flat concatenation of the tensors in canonical order (0 = zero padding), half_grp = scale group g (>= 0: the
 * "hi" half, f16(v * 2^k_g); < 0: the "lo" half of group -g-1, f16(v * 2^k_g - hi)), 2^k_g bringing the group's
 * largest |v| into [2^13, 2^14).  Per fp32 constant: c_code 0: flat[c_src - 1] * c_mult; 1: 2^-k_g; 2: 2^-k_g / 8
 * (g = c_group).  [host] arrays; returns the number of constants or a negative INERF_E_*. */
int64_t inerf_pack_map(const inerf_net_desc* net, int backward, int32_t* half_src, int32_t* half_grp, int64_t half_capacity,
                       int32_t* c_dst, int32_t* c_src, int32_t* c_group, int32_t* c_code, float* c_mult, int64_t const_capacity,
                       int32_t* n_groups);

/* The re-packing that inerf_pack_map describes, done by the library: params = n_tensors DEVICE pointers to the parameter
 * tensors in canonical order ([host] array; counts = their element counts), the map arrays uploaded to the device as int32
 * (half_src / half_grp: 2 * packed_floats entries; group_src: [n_groups, longest] flat indices (1-based, 0 = padding) of every
 * scale group's sources; the constants as returned), gmax_scratch: n_groups device floats.  Writes the packed blob
 * (packed_floats floats), bit-identical to inerf_pack_weights / inerf_pack_weights_bwd.  A memset and three launches. */
int inerf_repack(const float* const* params, const int64_t* counts, int n_tensors, const int32_t* half_src, const int32_t* half_grp,
                 int64_t packed_floats, const int32_t* group_src, int n_groups, int longest, const int32_t* c_dst,
                 const int32_t* c_src, const int32_t* c_grp, const int32_t* c_code, const float* c_mult, int n_consts,
                 float* gmax_scratch, float* packed_out, void* stream);

/* Alpha compositing.  Replaces raw2outputs: run_nerf.py:359-412 / model_utils.py:39-116.
 * raw[N,S,CH]; z[N,S]; rays_d: pointer to the first direction, consecutive rays `rays_d_stride`
 * floats apart (3 for a [N,3] tensor, 11 for the d-part of a packed ray batch);
 * noise[N,S] (already scaled by raw_noise_std) or NULL.  n_classes / feat_dim select the optional
 * semantic (raw[...,11:11+C]) and endpoint-feature (the LAST feat_dim channels) sums.
 * Any output pointer may be NULL to skip it.  disp is NaN where acc == 0, as in the reference.
 * Limits: 1 <= S <= INERF_MAX_SAMPLES (forward and backward); any CH >= 11 + n_classes + feat_dim. */
typedef struct inerf_composite_out {
    float* rgb;       /* [N,3] */
    float* disp;      /* [N]   */
    float* acc;       /* [N]   */
    float* depth;     /* [N]   */
    float* albedo;    /* [N,3] */
    float* shading;   /* [N]   */
    float* residual;  /* [N,3] */
    float* sem;       /* [N,C]        or NULL */
    float* feat;      /* [N,feat_dim] or NULL */
    float* weights;   /* [N,S]        or NULL */
} inerf_composite_out;

int inerf_composite(const float* raw, const float* z_vals, const float* rays_d, int rays_d_stride, const float* noise,
                    int64_t n_rays, int n_samples, int channels, int n_classes, int feat_dim, uint32_t flags,
                    const inerf_composite_out* out, void* stream);

/* Backward of the alpha compositing: d_raw[N,S,CH] = sum over the given output gradients of
 * d(output)/d(raw).  Replaces what autograd records for raw2outputs when the trainers call
 * loss.backward() (run_nerf.py:1018 through :359-412; trainer.py:990 through model_utils.py:39-116).
 * Same inputs as inerf_composite (the forward pass is recomputed, nothing has to be saved); `grads`
 * holds dL/d(output) for every output the loss used, NULL for the others (const pointers, the
 * struct is inerf_composite_out read as inputs; `weights` is dL/d weights[N,S]).  z_vals, rays_d
 * and noise get no gradient (the reference detaches the resampled depths, run_nerf.py:501, and the
 * rays are data).  Every element of d_raw is written (zero where nothing depends on it). */
int inerf_composite_backward(const float* raw, const float* z_vals, const float* rays_d, int rays_d_stride,
                             const float* noise, int64_t n_rays, int n_samples, int channels, int n_classes,
                             int feat_dim, uint32_t flags, const inerf_composite_out* grads, float* d_raw, void* stream);

/* Hierarchical resampling + merge.  Replaces z_vals_mid + sample_pdf + sort(cat(...)) + std:
 * run_nerf.py:499-503,519 + run_nerf_helpers.py:402-445 / trainer.py:758-766,799 + rays.py:176-220.
 * z_coarse[N,Sc], weights[N,Sc] (the full coarse weights; the kernel takes [1:-1] itself);
 * u: [n_importance] shared, or [N,n_importance] with INERF_FLAG_U_PER_RAY.
 * Outputs (any may be NULL): z_samples[N,n_importance], z_merged[N,Sc+n_importance] ascending,
 * z_std[N] (population std of the new samples).  Limits: INERF_MIN_COARSE (3) <= Sc <= INERF_MAX_COARSE (256),
 * 1 <= n_importance <= INERF_MAX_IMPORTANCE (512). */
int inerf_sample_fine(const float* z_coarse, const float* weights, const float* u, int64_t n_rays, int n_coarse,
                      int n_importance, uint32_t flags, float* z_samples, float* z_merged, float* z_std, void* stream);

/* Stand-alone inverse-CDF sampler with the reference's own signature sample_pdf(bins, weights, N):
 * run_nerf_helpers.py:402-445 / rays.py:176-220.  bins[N,n_bins], weights[N,n_bins-1],
 * u as above -> samples[N,n_samples].  Limits: INERF_MIN_BINS (2) <= n_bins <= INERF_MAX_COARSE (256),
 * 1 <= n_samples <= INERF_MAX_IMPORTANCE (512). */
int inerf_sample_pdf(const float* bins, const float* weights, const float* u, int64_t n_rays, int n_bins, int n_samples,
                     uint32_t flags, float* samples, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Whole path.  Replaces render_rays (run_nerf.py:415-528) / SSRTrainer.volumetric_rendering
 * (trainer.py:717-808) for one ray batch: coarse sampling -> coarse MLP -> compositing ->
 * resampling -> fine MLP -> compositing, all enqueued on `stream` with no host synchronisation.
 * ------------------------------------------------------------------------------------------- */
typedef struct inerf_render_args {
    /* networks */
    inerf_net_desc net;
    const float* packed_coarse;   /* device blob                                                   */
    const float* packed_fine;     /* device blob; NULL = reuse coarse (network_fine is None)        */
    /* inputs */
    const float* rays;            /* [N,11]                                                        */
    int64_t      n_rays;
    int32_t      n_samples;       /* coarse samples per ray                                        */
    int32_t      n_importance;    /* 0 = coarse pass only                                          */
    uint32_t     flags;           /* INERF_FLAG_*                                                  */
    const float* t_vals;          /* [n_samples] linspace(0,1,n_samples)                           */
    const float* t_rand;          /* [N,n_samples] or NULL                                         */
    const float* u;               /* [n_importance] or [N,n_importance] (INERF_FLAG_U_PER_RAY)     */
    const float* noise_coarse;    /* [N,n_samples] or NULL                                         */
    const float* noise_fine;      /* [N,n_samples+n_importance] or NULL                            */
    /* outputs (any pointer may be NULL) */
    inerf_composite_out coarse;
    inerf_composite_out fine;
    float* z_std;                 /* [N]                                                           */
    float* raw_coarse;            /* [N,n_samples,CHc]; NULL = keep in workspace                   */
    float* raw_fine;              /* [N,n_samples+n_importance,CHf]; NULL = keep in workspace      */
    float* z_coarse;              /* [N,n_samples]          optional copy-out of stage tensors     */
    float* z_samples;             /* [N,n_importance]                                               */
    float* z_fine;                /* [N,n_samples+n_importance]                                     */
    int32_t* status;              /* optional device word for INERF_STATUS_* bits (caller zeroes it) */
    int64_t  status_rays;         /* <= 0: one status word; > 0: ceil(n_rays / status_rays) words, one per that many rays
                                     (inerf_encode_mlp_chunked)                                     */
    /* scratch */
    void*   workspace;
    int64_t workspace_bytes;
    /* the probe's margin states (INERF_FLAG_GATE_PROBE; device, INERF_GATE_STATE_BYTES each, or NULL: the constant margin): of the
     * network the coarse pass evaluates and of the one the fine pass evaluates - with packed_fine NULL, the coarse network's in both */
    void* gate_state_coarse;
    void* gate_state_fine;
} inerf_render_args;

/* Bytes of workspace inerf_render_rays needs for these sizes when the caller supplies none of the optional stage
 * outputs (an upper bound for every call with these sizes). */
int64_t inerf_workspace_bytes(const inerf_net_desc* net, int64_t n_rays, int n_samples, int n_importance, uint32_t flags);

/* Bytes of workspace THIS call needs: stage tensors the caller supplies as outputs (raw_coarse, raw_fine, z_coarse,
 * z_samples, z_fine, coarse.weights) are written in place and get no workspace region - raw alone is N x S x CH
 * floats.  `workspace` / `workspace_bytes` of the argument are ignored.  May return 0 (workspace may then be NULL). */
int64_t inerf_render_workspace_bytes(const inerf_render_args* args);

/* Limits (the stage kernels' own, checked once before anything is enqueued - INERF_E_UNSUPPORTED): n_importance == 0:
 * n_samples <= INERF_MAX_SAMPLES; n_importance > 0: INERF_MIN_COARSE <= n_samples <= INERF_MAX_COARSE and
 * n_importance <= INERF_MAX_IMPORTANCE. */
int inerf_render_rays(const inerf_render_args* args, void* stream);

/* Raw channel counts for this network. */
int inerf_raw_channels(const inerf_net_desc* net, uint32_t flags, int fine);

/* ---------------------------------------------------------------------------------------------
 * Training draws: the random tensors of a training-mode render, drawn inside the kernels.
 * Replaces the stratified jitter t_rand[N,S] (run_nerf.py:472-486, trainer.py:737-746), the density noise
 * randn * raw_noise_std of both passes (run_nerf.py:386-387, model_utils.py:70-72) and the inverse-CDF variates u[N,Ni]
 * (run_nerf_helpers.py:410-414, rays.py:194-197).  A sample's draw is a pure function of (seed, step, stream, global ray index,
 * sample index): the same batch gives the same bits for any chunking and any split of the rays over callers, and a backward pass
 * regenerates the noise its forward added instead of keeping it.  (torch's own random streams are not reproduced.)
 *
 * Philox4x32-10 as Random123 defines it (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds):
 *   key     = {seed & 0xffffffff, seed >> 32}
 *   counter = {ray, block | (stream << 16), step & 0xffffffff, step >> 32}
 *     ray    = ray_base + the ray's index in this call, an unsigned 32-bit value;
 *     block  = sample >> 2: the four output words belong to samples 4 block .. 4 block + 3 (sample < INERF_MAX_SAMPLES, block < 256);
 *     stream = INERF_DRAW_STREAM_*.
 *   uniform (jitter, u):  (word >> 8) * 2^-24 - in [0, 1) on torch.rand's fp32 lattice, never 1.
 *   normal (the noise streams): Box-Muller on the word pairs (0, 1) and (2, 3):
 *     u1 = ((w_even >> 9) + 1) * 2^-23 in (0, 1], u2 = (w_odd >> 8) * 2^-24, r = sqrtf(-2 logf(u1)), theta = fp32(2 pi) * u2;
 *     the pair's even sample is r cosf(theta), its odd sample r sinf(theta) (accurate library functions); |z| < 5.65.
 *     The noise added to sigma is z * noise_std, rounded once, as randn * std is.
 * step: the host value, or *step_dev (DEVICE, one int64, 8-byte aligned) when that is not NULL.  No drawing kernel writes it:
 *   inerf_draw_advance is a launch of its own (one workgroup) that adds 1, so a captured step draws anew at every replay.
 * Every drawn entry point takes the arguments of its classic form plus an inerf_draw_args; the classic random-tensor pointers must be
 * NULL there (INERF_E_INVALID otherwise, as for a misaligned step_dev, a negative or non-finite noise_std or a flag that means nothing
 * to the entry point: INERF_DRAW_PERTURB is inerf_render_rays_drawn's alone, INERF_DRAW_FINE the two composite calls'), and
 * ray_base + n_rays > 2^32 is INERF_E_UNSUPPORTED - all checked before anything is enqueued, for an empty batch too.  A drawn call and
 * the classic call fed with inerf_draw_fill's tensors give the same bits.
 * ------------------------------------------------------------------------------------------- */
#define INERF_DRAW_STREAM_JITTER        0
#define INERF_DRAW_STREAM_NOISE_COARSE  1
#define INERF_DRAW_STREAM_U             2
#define INERF_DRAW_STREAM_NOISE_FINE    3
#define INERF_DRAW_PERTURB  1u   /* inerf_render_rays_drawn: perturb > 0 - jitter the coarse depths, per-ray random u            */
#define INERF_DRAW_FINE     2u   /* inerf_composite[_backward]_drawn: the fine pass's noise stream (3) instead of the coarse (1) */
typedef struct inerf_draw_args {
    uint64_t seed;
    int64_t step;
    const int64_t* step_dev;
    uint64_t ray_base;
    float noise_std;
    uint32_t flags;
} inerf_draw_args;

/* out[n_rays, n_per_ray] = one stream as the tensor the classic entry points take (the noise streams already scaled by noise_std):
 * the test instrument, and the way to look at what a drawn call used.  1 <= n_per_ray <= INERF_MAX_SAMPLES. */
int inerf_draw_fill(const inerf_draw_args* draw, int stream_id, int64_t n_rays, int n_per_ray, float* out, void* stream);
/* *step_dev += 1 (one workgroup, one plain store). */
int inerf_draw_advance(int64_t* step_dev, void* stream);

/* inerf_sample_coarse with the jitter drawn (stream 0); t_rand must be NULL.  n_samples <= INERF_MAX_SAMPLES. */
int inerf_sample_coarse_drawn(const float* rays, const float* t_vals, const float* t_rand, int64_t n_rays, int n_samples,
                              uint32_t flags, float* z_out, const inerf_draw_args* draw, void* stream);
/* inerf_composite / inerf_composite_backward with the noise regenerated (stream 1, or 3 with INERF_DRAW_FINE); noise must be NULL. */
int inerf_composite_drawn(const float* raw, const float* z_vals, const float* rays_d, int rays_d_stride, const float* noise,
                          int64_t n_rays, int n_samples, int channels, int n_classes, int feat_dim, uint32_t flags,
                          const inerf_composite_out* out, const inerf_draw_args* draw, void* stream);
int inerf_composite_backward_drawn(const float* raw, const float* z_vals, const float* rays_d, int rays_d_stride,
                                   const float* noise, int64_t n_rays, int n_samples, int channels, int n_classes,
                                   int feat_dim, uint32_t flags, const inerf_composite_out* grads, float* d_raw,
                                   const inerf_draw_args* draw, void* stream);
/* inerf_sample_fine / inerf_sample_pdf with per-ray u drawn (stream 2; the unsorted-u path of INERF_FLAG_U_PER_RAY); u must be NULL. */
int inerf_sample_fine_drawn(const float* z_coarse, const float* weights, const float* u, int64_t n_rays, int n_coarse,
                            int n_importance, uint32_t flags, float* z_samples, float* z_merged, float* z_std,
                            const inerf_draw_args* draw, void* stream);
int inerf_sample_pdf_drawn(const float* bins, const float* weights, const float* u, int64_t n_rays, int n_bins, int n_samples,
                           uint32_t flags, float* samples, const inerf_draw_args* draw, void* stream);
/* inerf_render_rays in training mode without an RNG of the caller's: t_rand, noise_coarse and noise_fine of `args` must be NULL.
 * INERF_DRAW_PERTURB (perturb > 0): the coarse depths are jittered and u is drawn per ray - args->u must be NULL; without it nothing
 * is drawn that the reference does not draw: args->u is the caller's (shared linspace) u as in the classic form.  noise_std > 0
 * (raw_noise_std): both passes add drawn noise - and are then not gated, as a pass with a noise tensor is not. */
int inerf_render_rays_drawn(const inerf_render_args* args, const inerf_draw_args* draw, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Image-level neighbours of the path.
 * ------------------------------------------------------------------------------------------- */

/* Ray generation: the [n_poses * height * width, 11] ray batch [o3, d3, near, far, viewdir3] of a pinhole camera.
 * Replaces get_rays (run_nerf_helpers.py:359-368) + the view-direction normalisation and concatenation inside
 * render() (run_nerf.py:99-128), and get_rays_camera / get_rays_world / create_rays (SSR/models/rays.py:27-67,
 * 223-256, depth_type "z").  poses: device, camera-to-world matrices as rows of 4 floats ([3,4] or [4,4] row-major),
 * consecutive poses `pose_stride` (>= 12) floats apart; static_poses: NULL, or the c2w_staticcam of the reference
 * (origins and directions from it, view directions from `poses`).  Pixel (i = column, j = row) of pose b is ray
 * b*H*W + j*W + i.  INERF_CAM_OPENGL: dirs = ((i-cx)/fx, -(j-cy)/fy, -1) (object-level, SSR convention "opengl");
 * otherwise ((i-cx)/fx, (j-cy)/fy, 1) (SSR "opencv").  Bit-identical to the reference's CPU evaluation
 * (tests/golden/rays_generators.npz): every fp32 operation is issued in ATen's order (see csrc/frame_ops.hip). */
#define INERF_CAM_OPENGL 1u
int inerf_gen_rays(const float* poses, int pose_stride, const float* static_poses, int n_poses, int height, int width,
                   float fx, float fy, float cx, float cy, float near, float far, uint32_t flags, float* rays_out,
                   void* stream);

/* The NDC projection of forward-facing scenes (ndc_rays, run_nerf_helpers.py:381-399), as render() applies it to the origin
 * and direction of every ray of the LLFF configs (run_nerf.py:117-119: ndc_rays(H, W, K[0][0], 1., rays_o, rays_d)).
 *   sx = -1./(W/(2.*focal)), sy = -1./(H/(2.*focal)) (run_nerf_helpers.py:387-393, evaluated by the caller and rounded to
 *   fp32 once, which is what ATen does with a Python scalar); near_plane = the `near` argument of ndc_rays.
 * Every fp32 operation is issued in ATen's CPU order (csrc/frame_ops.hip): t = (-(near + o_z)) / d_z, o' = o + t d without
 * fma, every quotient a true division, and `scalar / o'_z` as the correctly rounded reciprocal times the scalar that
 * Tensor.__rtruediv__ evaluates.  Bit-identical to the reference's CPU rays (tests/golden/rays_generators.npz: ndc_o, ndc_d,
 * render_rays_ndc; tests/golden/uncurated_object_llff_ndc.npz: rays). */
typedef struct inerf_ndc { float sx, sy, near_plane; } inerf_ndc;          /* [host] */

/* inerf_gen_rays with the NDC projection of run_nerf_helpers.py:381-399 applied to origin and direction
 * (run_nerf.py:117-119); view directions stay the world-space direction of `poses` over its norm (run_nerf.py:101-108),
 * with static_poses origin and direction - and so the NDC of them - come from the static camera; near / far are columns 6
 * and 7 as given.  ndc == NULL: exactly inerf_gen_rays. */
int inerf_gen_rays_ndc(const float* poses, int pose_stride, const float* static_poses, int n_poses, int height, int width,
                       float fx, float fy, float cx, float cy, float near, float far, uint32_t flags,
                       const inerf_ndc* ndc, float* rays_out, void* stream);

/* The [n, 11] batch render() assembles from GIVEN rays (run_nerf.py:106-128; every object-level training step,
 * run_nerf.py:942): view direction = d / |d| with |d| = sqrt(fma(d2, d2, fma(d1, d1, d0 * d0))) (torch.norm on the CPU) and
 * a true division, optional NDC of origin and direction (ndc NULL: none), near / far columns.  rays_o / rays_d: rows of three
 * floats, consecutive rows o_stride / d_stride (>= 3) floats apart - columns 0:3 and 3:6 of an [n, 11] batch go in as they
 * are.  rays_out must not overlap the inputs.  INERF_E_UNSUPPORTED beyond (2^31 - 1) * 256 rays. */
int inerf_assemble_rays(const float* rays_o, int64_t o_stride, const float* rays_d, int64_t d_stride, int64_t n_rays,
                        float near, float far, const inerf_ndc* ndc /* or NULL */, float* rays_out, void* stream);

/* ndc_rays alone (run_nerf_helpers.py:381-399): contiguous [n, 3] outputs; o_out / d_out may alias rays_o / rays_d when
 * those are contiguous (stride 3).  ndc must not be NULL. */
int inerf_ndc_rays(const float* rays_o, int64_t o_stride, const float* rays_d, int64_t d_stride, int64_t n_rays,
                   const inerf_ndc* ndc, float* o_out, float* d_out, void* stream);

/* to8b on the device: out[i] = (uint8)(255 * clip(values[i], 0, 1)) (run_nerf_helpers.py:13 / trainer.py:1242), so an
 * image loop (run_nerf.py:142-212, trainer.py:1221-1389) copies a quarter of the bytes to the host.  NaN -> 0. */
int inerf_frame_to_u8(const float* values, int64_t n, unsigned char* out, void* stream);

/* Nearest-anchor lookup of the albedo clustering, every semantic class in one launch.  Replaces
 * Cluster_Manager.dest_color / dest_class (SSR/training/cluster.py:73-98) and, underneath, Cluster.dest_color /
 * dest_class (:275-297), mapping_color (:324-330), compute_dist (:299-305) and nearest_anchor (:307-310); called
 * once per training step (trainer.py:913-920) and once per rendered frame (:1427-1430).
 *   rgb[n,3]; label[n] (int64; ignored - may be NULL - with INERF_CLUSTER_IGNORE_LABEL, the reference's
 *   class_num == 1 shortcut of dest_color, cluster.py:75-77);
 *   anchors[A,4] = {a0, a1, a2, a0^2+a1^2+a2^2} in the mapped colour space, 16-byte aligned, the classes' anchors
 *   back to back: class c owns rows anchor_begin[c] .. anchor_begin[c+1] (an empty range = the reference's
 *   `clusters[c] is None`); links[A] = centre of each anchor, relative to its class (int32);
 *   factor[K] = intensity_factor of each class's cluster; centers[Ctot,3] = rgb_centers back to back, class c
 *   starting at row center_begin[c].  All device pointers.
 * Outputs (either may be NULL): out_color[n,3] = rgb_centers[links[argmin]] of the pixel's class - the pixel itself
 * where its label has no cluster or lies outside [0, K); out_class[n] (int64) = links[argmin], 0 for those pixels.
 * argmin follows torch: the first minimal index wins, NaN distances (zero-intensity pixels) count as minimal. */
#define INERF_CLUSTER_IGNORE_LABEL 1u
int inerf_cluster_lookup(const float* rgb, const int64_t* label, int64_t n_pixels, const float* anchors,
                         const int32_t* links, const int32_t* anchor_begin, const float* factor, const float* centers,
                         const int32_t* center_begin, int n_classes, uint32_t flags, float* out_color,
                         int64_t* out_class, void* stream);

/* Mean-shift fitting of the albedo clusters, every semantic class of a manager in one call: the tables that
 * inerf_cluster_lookup reads.  Replaces Cluster_Manager.update_center (SSR/training/cluster.py:52-70) and, per class,
 * Cluster.update_center (:138-152): mapping_color_np, sklearn's estimate_bandwidth(quantile, n_samples, random_state=0),
 * max(bw * band_factor, 0.01), MeanShift(bandwidth, bin_seeding=True).fit, choose_anchors (:156-182) and
 * inv_mapping_color (:335-341).
 *   pixels[n,3] rgb; labels[n] int64 (NULL: every pixel belongs to class 0, the SSR class_num == 1 path; labels outside
 *   [0, K) belong to no class).  Class c's pixels are taken in their original order.
 *   sample_idx = the estimate_bandwidth subsample of every class, back to back: class c's indices (into the class's
 *   pixels, in that order) are sample_idx[sample_begin[c] .. sample_begin[c+1]), i.e.
 *   RandomState(0).permutation(n_c)[:n_samples] computed by the caller; max_class_samples = the largest such range
 *   (at most 8192).  factor[K] = intensity_factor of each class.  All arrays are device pointers.
 * Outputs (device): out_bandwidth[K] (0 for a class without pixels); out_center_begin[K+1] / out_centers[n,3] (rgb
 *   centres, clamped to [0,1]); out_anchor_begin[K+1] / out_anchors[n,3] / out_links[n] (int64, centre index inside the
 *   class) - every array sized for n rows, class c owning rows begin[c] .. begin[c+1].  Optional (may be NULL):
 *   out_mapped_centers[n,3] (cluster_centers_ in the mapped space), out_center_counts[n] (points within bw of each
 *   centre), out_pixel_label[n] (labels_ of every pixel in its class, -1 outside every class), out_class_stats[K,4]
 *   (pixels, seeds, non-empty seeds, centres).  status[4] (device int32): status[0] bit 1 = a non-finite mapped colour,
 *   bit 2 = a mapped colour of magnitude >= 256 (unsupported), bit 4 = a sample index outside its class; the outputs are
 *   meaningless when it is not 0.  Limits: n < 2^24, K <= 255 (INERF_E_UNSUPPORTED beyond). */
typedef struct inerf_cluster_fit_args {
    const float* pixels;
    const int64_t* labels;
    int64_t n_pixels;
    int32_t n_classes;
    int32_t max_class_samples;
    const int32_t* sample_idx;
    const int32_t* sample_begin;
    int64_t n_sample_idx;
    const float* factor;
    double quantile;
    double band_factor;
    void* workspace;
    int64_t workspace_bytes;
    double* out_bandwidth;
    float* out_centers;
    int32_t* out_center_begin;
    float* out_anchors;
    int64_t* out_links;
    int32_t* out_anchor_begin;
    float* out_mapped_centers;
    int32_t* out_center_counts;
    int32_t* out_pixel_label;
    int32_t* out_class_stats;
    int32_t* status;
} inerf_cluster_fit_args;
/* workspace of inerf_cluster_fit in bytes (negative INERF_E_* for bad sizes); n_sample_idx = total subsample indices */
int64_t inerf_cluster_fit_workspace_bytes(int64_t n_pixels, int n_classes, int64_t n_sample_idx);
int inerf_cluster_fit(const inerf_cluster_fit_args* args, void* stream);

/* Cluster refresh on the device: the pass of render_path(update_cluster=True) (run_nerf.py:142-272, trainer.py:1221-1443)
 * either side of inerf_cluster_fit.
 *
 * inerf_frame_subsample: the fit's sample set of one rendered frame.  frame = the frame's maps side by side, one row of
 *   `row_stride` floats per pixel (frames.pack_maps), height * width rows.  Every pixel (r, c) with r % step == 0 and
 *   c % step == 0, in row-major order - albedos[-1][::step, ::step, :].reshape(-1, 3) (run_nerf.py:176, trainer.py:1287) -
 *   writes its columns albedo_col .. albedo_col + 2 to out_pixels[row, 3] and, with label_col >= 0, its label column
 *   (a float holding an exact small integer, truncated to int64) to out_labels[row]; the caller passes both pointers
 *   already advanced to the frame's place in the table.  ceil(height / step) * ceil(width / step) rows are written.
 *   With label_col >= 0 and class_counts != NULL every label in [0, n_classes) also adds one to class_counts[label]
 *   (int32, zeroed by the caller once per pass): np.bincount(lab[(lab >= 0) & (lab < K)], minlength=K), integer atomics.
 *   label_col = -1: out_labels and class_counts are not touched (may be NULL).
 *   INERF_E_INVALID: a negative height or width, step < 1, a null frame / out_pixels (/ out_labels with a label column),
 *   a column outside the row, n_classes < 1 with counts, pointers not aligned to their element; a zero-sized frame is
 *   INERF_OK whatever the pointers; INERF_E_UNSUPPORTED: more than 2^31 - 1 blocks of 256 rows. */
int inerf_frame_subsample(const float* frame, int64_t row_stride, int albedo_col, int label_col, int height, int width, int step,
                          float* out_pixels, int64_t* out_labels, int32_t* class_counts, int n_classes, void* stream);

/* inerf_cluster_snap_compose: dest_color of every pixel of a frame and the two 8-bit images the pass writes from it
 *   (run_nerf.py:226-241, trainer.py:1425-1440).  albedo (3 floats), label (1 float, an exact small integer truncated to
 *   int64; ignored - may be NULL - with INERF_CLUSTER_IGNORE_LABEL), shading (1 float) and residual (3 floats) point at
 *   the first pixel's values; consecutive pixels are `row_stride` floats apart for all four (columns of one packed frame).
 *   The cluster tables are inerf_cluster_lookup's, and so are the search, its argmin and its NaN rule:
 *     snapped = rgb_centers[links[argmin]] of the pixel's class - the albedo itself where its label has no cluster
 *     out_c[n,3]    = to8b(snapped)
 *     out_edit[n,3] = to8b(snapped * shading + residual)   one fp32 product, one fp32 sum, as numpy rounds them
 *   to8b as inerf_frame_to_u8: (uint8)(255 * clip(x, 0, 1)), NaN -> 0.  out_color[n,3] (fp32, optional, may be NULL)
 *   receives `snapped`; without it neither the float colour nor the float edit image is written anywhere.
 *   INERF_E_INVALID: a null pointer (out_color excepted), n_pixels < 0, row_stride < 3, n_classes < 1, anchors not
 *   16-byte aligned, any other pointer - out_c and out_edit included - not 4-byte aligned; n_pixels == 0 is INERF_OK
 *   whatever the pointers; INERF_E_UNSUPPORTED: more than 2^31 - 1 blocks. */
int inerf_cluster_snap_compose(const float* albedo, const float* label, const float* shading, const float* residual,
                               int64_t row_stride, int64_t n_pixels, const float* anchors, const int32_t* links,
                               const int32_t* anchor_begin, const float* factor, const float* centers,
                               const int32_t* center_begin, int n_classes, uint32_t flags, unsigned char* out_c,
                               unsigned char* out_edit, float* out_color, void* stream);

/* Scene editing on the device: the edit engine of the reference's GUI (gui.py; gui_obj.py is the same engine) - recolour a
 * cluster centre, reshape and rescale shading and residual, compose the frame again.
 *
 * inerf_edit_params: the edit state both kernel forms read (host struct, passed by pointer, copied at the call).
 *   edit_centers[Ctot,3] (device, fp32) = the editable copy of inerf_cluster_lookup's `centers`, same layout: rgb_centers of
 *   gui.py:49-60 (update_color) / :337-352 (reset); shading_mode 0: t_shading(s) = s, 1: s * s (gui.py:490-496);
 *   residual_mode 0: t_residual(r) = r, 1: (sin(r * pi - pi / 2) + 1) / 2 (gui.py:498-502), pi and pi / 2 rounded to fp32
 *   first, the accurate sine; shading_scale, residual_scale = global_shading_scale, global_residual_scale (gui.py:478-488).
 *   Per pixel and channel (gui.py:163, fp32, left to right, no contraction):
 *     result = ((colour * t_shading(shading)) * shading_scale) + (t_residual(residual) * residual_scale)
 *   8-bit outputs are to8b as inerf_frame_to_u8: (uint8)(255 * clip(x, 0, 1)), NaN -> 0. */
typedef struct inerf_edit_params {
    const float* edit_centers;
    int32_t shading_mode;
    int32_t residual_mode;
    float shading_scale;
    float residual_scale;
} inerf_edit_params;

/* inerf_edit_frame: search form, for a frame seen for the first time - cluster_img (gui.py:268-281, :529-540) and
 *   update_img (gui.py:155-163) in one launch.  Inputs and cluster tables are inerf_cluster_snap_compose's (`centers` is
 *   replaced by params->edit_centers), and so are the search, its argmin, its NaN rule and its two tile widths:
 *     colour = edit_centers[center_begin[label] + links[argmin]] - the albedo itself where the label has no cluster
 *     out_result[n,3] (u8) = to8b(result); out_c[n,3] (u8, optional) = to8b(colour) (view mode 1, gui.py:171-173);
 *     out_result_f32[n,3] (optional) = result; out_slot[n] (int32, optional) = center_begin[label] + links[argmin], the
 *     global row of the pixel's centre, or -1 where the pixel keeps its albedo (label outside [0, K), class without cluster).
 *   INERF_E_INVALID: a null required pointer (params and its edit_centers included), n_pixels < 0, row_stride < 3,
 *   n_classes < 1, a mode outside {0, 1}, anchors not 16-byte aligned, any other pointer - out_result and out_c included -
 *   not 4-byte aligned; n_pixels == 0 is INERF_OK whatever the pointers; INERF_E_UNSUPPORTED: more than 2^31 - 1 blocks. */
int inerf_edit_frame(const float* albedo, const float* label, const float* shading, const float* residual, int64_t row_stride,
                     int64_t n_pixels, const float* anchors, const int32_t* links, const int32_t* anchor_begin,
                     const float* factor, const int32_t* center_begin, int n_classes, uint32_t flags,
                     const inerf_edit_params* params, unsigned char* out_result, unsigned char* out_c, float* out_result_f32,
                     int32_t* out_slot, void* stream);

/* inerf_edit_recompose / inerf_edit_recompose_u8: cached form, every later tick of update_img (gui.py:155-163) - no search.
 *   colour = slot[p] >= 0 ? edit_centers[slot[p]] : albedo[p]; then the same transfers, scales and outputs as above.
 *   Sources: fp32 pack columns as above (albedo 3, shading 1, residual 3 floats, consecutive pixels row_stride floats apart),
 *   or the three 8-bit planes load_all_image reads (gui.py:216-228) - albedo[n,3], shading[n], residual[n,3] - converted as
 *   (float)v / 255.0f, IEEE division = numpy's (v / 255.).astype(float32) for all 256 values.
 *   n_pixels may span a whole sequence of frames back to back.  8-bit sources and out_result / out_c are taken at ANY byte
 *   alignment (a frame of an odd pixel count inside a sequence): whole dwords in the middle, bytes at head and tail.
 *   INERF_E_INVALID: a null required pointer (out_c, out_result_f32 are optional), n_pixels < 0, a mode outside {0, 1},
 *   row_stride < 3 (fp32 form), slot / fp32 pointers / edit_centers not 4-byte aligned; n_pixels == 0 is INERF_OK whatever
 *   the pointers; INERF_E_UNSUPPORTED: more than 2^31 - 1 blocks of 2048 pixels. */
int inerf_edit_recompose(const float* albedo, const float* shading, const float* residual, int64_t row_stride, const int32_t* slot,
                         int64_t n_pixels, const inerf_edit_params* params, unsigned char* out_result, unsigned char* out_c,
                         float* out_result_f32, void* stream);
int inerf_edit_recompose_u8(const unsigned char* albedo, const unsigned char* shading, const unsigned char* residual,
                            const int32_t* slot, int64_t n_pixels, const inerf_edit_params* params, unsigned char* out_result,
                            unsigned char* out_c, float* out_result_f32, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Networks outside the fused architecture, and fp32 training batches: one launch per nn.Linear on the fp32 matrix core.
 *
 * The reference builds NeRF(D=args.netdepth, W=args.netwidth, skips, use_viewdirs) / Semantic_NeRF(...) from its flags
 * (object_level/run_nerf.py:286-296, SSR/training/trainer.py:811-846); the fused kernels above implement D=8, W=256,
 * skips=[4].  These entry points evaluate ANY such network layer by layer (object_level/run_nerf_helpers.py:284-321,
 * SSR/models/semantic_nerf.py:120-181: every F.linear / F.relu / F.sigmoid / torch.cat of the two forwards) and what
 * loss.backward() records for those layers (run_nerf.py:1018, trainer.py:990), in exact fp32 (v_mfma_f32_32x32x2_f32,
 * fp32 accumulate), activations in caller-owned HBM buffers.  The Python mirrors also use them for a training batch whose
 * activations leave the f16 range of the split-precision kernels, so no ATen GEMM remains on the path.
 * --------------------------------------------------------------------------------------------------------------- */
#define INERF_ACT_NONE     0
#define INERF_ACT_RELU     1   /* F.relu: negative -> 0, NaN stays NaN */
#define INERF_ACT_SIGMOID  2   /* torch.sigmoid: 1 / (1 + exp(-x)), IEEE division */

/* C[i, j] = epilogue(sum_k A(i, k) B(j, k)),  i < m, j < n, k < k:
 *   A(i, k) = a[i * a_sm + k * a_sk], B(j, k) = b[j * b_sn + k * b_sk]; each operand needs ONE unit stride (either one);
 *   epilogue, in this order: + bias[j] (if not NULL), + add[i * add_ld + j] (if not NULL; add == c accumulates), act,
 *   then zeroed where gate[i * gate_ld + j] <= 0 (if gate is not NULL: the ReLU backward of the layer that produced `gate`);
 *   c[i * c_ld + j] may be a column range of a wider buffer (that is how torch.cat([input_pts, h]) and
 *   torch.cat([feature, input_views]) are formed, run_nerf_helpers.py:291,308).
 * nn.Linear forward: a = X (a_sm = ld, a_sk = 1), b = weight (b_sn = in_features, b_sk = 1), m = points, n = out, k = in.
 * Its input gradient:  a = dZ (a_sm = ld, a_sk = 1), b = weight (+ first input column), b_sn = 1, b_sk = in_features,
 *                      n = input columns, k = out_features. */
typedef struct inerf_linear_args {
    const float* a; int64_t a_sm, a_sk;
    const float* b; int64_t b_sn, b_sk;
    const float* bias;
    const float* add; int64_t add_ld;
    const float* gate; int64_t gate_ld;
    float* c; int64_t c_ld;
    int64_t m; int32_t n; int32_t act; int64_t k;
} inerf_linear_args;
int inerf_linear(const inerf_linear_args* args, void* stream);

/* d_weight[rows, cols] (=|+=) sum_p g[p, r] x[p, c];  d_bias[rows] (=|+=) sum_p g[p, r]  (NULL: not wanted) - what autograd
 * accumulates into nn.Linear.weight.grad / .bias.grad for g = the gradient of the layer's output (already multiplied by the
 * activation's derivative), x = its input.  g[p * ldg + r], x[p * ldx + c].  Split over the points into a fixed number of
 * partial products (workspace: inerf_linear_wgrad_workspace_bytes), added in ascending order: bit-identical run to run. */
int64_t inerf_linear_wgrad_workspace_bytes(int64_t n_points, int rows, int cols);
int inerf_linear_wgrad(const float* g, int64_t ldg, int rows, const float* x, int64_t ldx, int cols, int64_t n_points,
                       float* d_weight, float* d_bias, int accumulate, void* workspace, int64_t workspace_bytes, void* stream);

/* Embedder.embed (run_nerf_helpers.py:195-225; semantic_nerf.py:50-66 with divisor = scalar_factor) into
 * out[p * ld + 0 .. 3 + 6 n_freqs): [x, sin(x), cos(x), sin(2x), cos(2x), ...] of x = (o + d * z[p]) / divisor
 * (run_nerf.py:488), or of the ray's view direction when `directions` != 0 (z_vals may then be NULL); p = ray * n_samples + s. */
int inerf_embed(const float* rays, const float* z_vals, int64_t n_rays, int n_samples, int n_freqs, float divisor, int directions,
                float* out, int64_t ld, void* stream);

/* raw[p, 0:3] = raw[p, 4:7] * raw[p, 7] + raw[p, 8:11] (rgb = albedo * shading + residual, run_nerf_helpers.py:319) and its
 * backward together with the three sigmoids': dz[p, 0:3] / [3] / [4:7] = gradients of the PRE-sigmoid albedo / shading /
 * residual given d_raw (the gradient of all raw channels) and raw (the forward's values); dz is [n_points, 8], dz[p, 7] = 0. */
int inerf_intrinsic_combine(float* raw, int64_t ld, int64_t n_points, void* stream);
int inerf_intrinsic_combine_backward(const float* raw, const float* d_raw, int64_t ld, int64_t n_points, float* dz, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The training losses of both trainers: every term of a step in ONE forward launch, every gradient in ONE backward launch.
 *
 * Replaces compute_intrinsic_loss (object_level/run_nerf_helpers.py:59-86, SSR/training/training_utils.py:179-207) with the
 * helpers under it (compute_chroma_loss, compute_residual_loss, compute_chroma_weight, compute_reflect_sparsity_loss,
 * compute_shading_smooth_loss, compute_intensity_loss: run_nerf_helpers.py:15-57, training_utils.py:127-176), img2mse
 * (run_nerf_helpers.py:11, training_utils.py:124) on the image (run_nerf.py:976,1006; trainer.py:923,936) and on the cluster
 * target (run_nerf.py:987,1012; trainer.py:985-986), nn.CrossEntropyLoss(ignore_index=-1) on label-1 (trainer.py:858-865,
 * 927,939), and what loss.backward() records for all of them (run_nerf.py:1018, trainer.py:990).  compute_depth_weight is
 * evaluated by the reference and then replaced by the literal 1 (run_nerf_helpers.py:78-84): disp and acc are not inputs.
 *
 * n_levels = 1 (one compute_intrinsic_loss call) or 2 (coarse = level 0 and fine = level 1 of one step); the levels share
 * gt_rgb, pair_key, cluster_target and ce_labels.  Pairing: split = n/2, ray i < split pairs with ray i + (n - split) (an odd n
 * leaves the middle ray unpaired); split2 = split/2, ray i < split2 pairs with ray i + (split - split2) (the "far" term).
 *   pair_key: float mask[n] (target_m, run_nerf.py:703), or with INERF_LOSS_KEY_LABELS int64 labels[n] compared as integers
 *     (training_utils.py:148) - the shading weight is then unmasked (training_utils.py:150).
 *   INERF_LOSS_MASK_OUTER: the mask was [n,1]; the reference's broadcast then forms a [split,split] matrix whose mean is
 *     mean(mask product) * mean(weight * distance) for the sparsity, shading and far terms: that factorised form is computed.
 *   level[l].rgb (optional, both levels or none): adds img2mse(rgb, gt_rgb).  cluster_target[n,3] (optional): adds
 *     img2mse(albedo, cluster_target).  level[l].logits[n, n_classes] + ce_labels[n] int64 (optional, both or none; n_classes
 *     in 1..INERF_LOSS_MAX_CLASSES): adds the cross-entropy; ce_label_offset is added to every label first (-1 = the
 *     reference's label-1 taken from the unshifted labels, 0 = already shifted); a label outside [0, n_classes) afterwards
 *     is ignored, the mean is taken over the others (none left: NaN, as torch).
 * state (device, inerf_intrinsic_loss_workspace_bytes): written by the forward, read by the backward -
 *   state[l*16 + t], t = INERF_LOSS_TERM_*: the terms of level l (absent ones 0), then [9] rgb_mean - albedo_mean, [10] / [11]
 *   mean mask product of the near / far pairs, [12] number of rays the cross-entropy counted;
 *   state[n_levels*16] = the weighted total sum_l sum_t weights[t] * term[l][t] over the terms that are present.
 * weights[INERF_LOSS_TERMS] (device; NULL = all 1).  An empty mean is NaN as in torch (n < 4: the far term; n < 2: the pair terms).
 * Backward: d(sum_l sum_t (grad_total[0] * weights[t] + grad_terms[l*INERF_LOSS_STATE_FLOATS + t]) * term[l][t]) with respect to every
 *   differentiable input (grad_total, grad_terms: device, either may be NULL); d_albedo[n,3], d_shading[n], d_residual[n,3] are
 *   required, d_rgb[n,3] / d_logits[n,n_classes] where the forward had rgb / logits.  One thread per ray gathers its own
 *   contributions (no atomics); both launches are bit-identical from run to run and read nothing on the host. */
#define INERF_LOSS_KEY_LABELS   1u
#define INERF_LOSS_MASK_OUTER   2u
#define INERF_LOSS_TERMS        9
#define INERF_LOSS_TERM_CHROMA    0
#define INERF_LOSS_TERM_RESIDUAL  1
#define INERF_LOSS_TERM_SPARSITY  2
#define INERF_LOSS_TERM_SHADING   3
#define INERF_LOSS_TERM_FAR       4
#define INERF_LOSS_TERM_INTENSITY 5
#define INERF_LOSS_TERM_IMAGE     6
#define INERF_LOSS_TERM_CLUSTER   7
#define INERF_LOSS_TERM_SEMANTIC  8
#define INERF_LOSS_STATE_FLOATS   16   /* per level */
#define INERF_LOSS_MAX_CLASSES    101
typedef struct inerf_loss_level {
    const float* albedo;
    const float* shading;
    const float* residual;
    const float* rgb;
    const float* logits;
    float* d_albedo;
    float* d_shading;
    float* d_residual;
    float* d_rgb;
    float* d_logits;
} inerf_loss_level;
typedef struct inerf_loss_args {
    int64_t n_rays;
    int32_t n_levels;
    int32_t n_classes;
    uint32_t flags;
    int32_t ce_label_offset;
    const float* gt_rgb;
    const void* pair_key;
    const float* cluster_target;
    const int64_t* ce_labels;
    const float* weights;
    const float* grad_total;
    const float* grad_terms;
    inerf_loss_level level[2];
    float* state;
    int64_t state_bytes;
} inerf_loss_args;
/* bytes of `state` (negative INERF_E_* for bad sizes) */
int64_t inerf_intrinsic_loss_workspace_bytes(int64_t n_rays, int n_levels);
int inerf_intrinsic_loss(const inerf_loss_args* args, void* stream);
int inerf_intrinsic_loss_backward(const inerf_loss_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Parameter update: one Adam step of a list of fp32 tensors.
 * Replaces optimizer.step() of the torch.optim.Adam both trainers build (object_level/run_nerf.py:304,1019;
 * SSR/training/trainer.py:842,991): weight_decay = 0, amsgrad = False, maximize = False.  Per element, in fp32 with one
 * rounding per operation (true division, correctly rounded square root - torch's eager single-tensor form):
 *     m = m + (1 - beta1) * (g - m)          (one fused multiply-add, as ATen's lerp kernels form it)
 *     v = v * beta2 + ((1 - beta2) * g) * g
 *     p = p - (lr / (1 - beta1^t)) * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps))
 * with 1 - beta1^t, sqrt(1 - beta2^t) and lr / (1 - beta1^t) formed in fp64 on the device and rounded to fp32 once per
 * tensor, as the eager path forms them in Python doubles.  t is the tensor's own step count AFTER its increment.
 *   params, grads, exp_avg, exp_avg_sq, steps: [host] arrays of n_tensors DEVICE pointers; tensor i has counts[i] (> 0)
 *     contiguous floats and may start on any 4-byte boundary (16-byte accesses are used where the four arrays of a tensor
 *     share their offset from a 16-byte boundary).  steps[i]: one fp32 on the device per tensor (torch's capturable layout),
 *     exact up to 2^24; the call advances it by 1.  No two entries may alias.
 *   counts: [host] array of n_tensors element counts.
 *   lr: the learning rate, taken in fp32 - unless lr_dev (DEVICE, one fp32) is non-NULL, which then wins: what a captured
 *     graph needs, since both trainers decay the rate every iteration (run_nerf.py:1024-1027, trainer.py:1006-1009).  Both
 *     forms are the same arithmetic, so a step launched directly and one replayed from a graph agree bit for bit.
 *   beta1, beta2 in [0, 1), eps > 0: fp64, as torch holds them (1 - beta is formed in fp64, then rounded).
 * The pointer table travels in the kernel arguments (no host-to-device copy): 72 tensors per table, a longer list takes
 * ceil(n_tensors / 72) tables.  Per table two launches: one workgroup advances the step counts, then one streaming launch
 * updates every tensor of the table (28 B per element; no atomics, no communication between workgroups; bit-identical from run
 * to run).  Nothing is allocated, synchronised or read on the host; capturable into a HIP graph.
 * Returns INERF_E_INVALID for a null or misaligned pointer, a non-positive count, a beta outside [0, 1) or eps <= 0 - every
 * check runs before the first launch - and INERF_OK with nothing launched for n_tensors == 0. */
typedef struct inerf_adam_args {
    int32_t n_tensors;
    float* const* params;
    const float* const* grads;
    float* const* exp_avg;
    float* const* exp_avg_sq;
    float* const* steps;
    const int64_t* counts;
    float lr;
    const float* lr_dev;
    double beta1;
    double beta2;
    double eps;
} inerf_adam_args;
int inerf_adam_step(const inerf_adam_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training batch assembly: from a pixel draw to the finished batch, one thread per selected pixel.
 * Replaces the first part of an iteration of both trainers: object_level/run_nerf.py:886-938 (img_i, get_rays, the coords
 * meshgrid, np.random.choice(replace=False), select_neighbor and the gathers that give batch_rays / target_s / target_m) and
 * SSR/training/trainer.py:627-691 with no_batching=True (sampling_index, rays.py:153-172, and the gathers that give
 * sampled_rays / gt_rgb / gt_depth / gt_semantic).  The 2n output rows are the n selected pixels followed by their n neighbours.
 *
 * Pixels.  INERF_BATCH_OBJECT: pixel q of the window [row0, row0 + win_h) x [col0, col0 + win_w) (the whole frame, or the centre
 *   crop H/2 +- dH, W/2 +- dW of run_nerf.py:902-909, computed by the caller) is (row0 + q / win_w, col0 + q % win_w).
 *   INERF_BATCH_SSR: q is the flat pixel h * width + w of the frame (the window fields are ignored).
 *   Neighbour: (row + off_row, col + off_col), each clamped to the IMAGE ([0, height-1], [0, width-1]), never to the window.
 * Rays.  OBJECT: out_rays is [2, 2n, 3], origins then directions, computed from poses[image] with k_gen_rays' operation order
 *   (bit-identical to get_rays followed by the reference's gather; no whole-frame table is built).  SSR: out_rays is [2n, 11]:
 *   rows of ray_table [n_images, H*W, 11] when it is non-NULL, else the rows inerf_gen_rays writes for poses / fx..far.
 *   INERF_BATCH_OPENGL selects the camera convention of computed rays (INERF_CAM_OPENGL; the object level always sets it).
 * Tables (all device-resident, contiguous):
 *   images [n_images, H, W, 3], image_bytes 4 (fp32) or 8 (fp64; SSR only - the SSR trainers hold fp64 images and depths);
 *     out_rgb [2n, 3] has the same element type.
 *   aux: OBJECT masks [n_images, H, W, 1] fp32 -> out_aux [2n, 1]; SSR depth [n_images, H, W], aux_bytes 4 or 8 -> out_aux [2n].
 *     Optional (NULL: not gathered).
 *   semantic (SSR, optional) [n_images, H, W], semantic_bytes 1 (uint8), 2, 4 or 8 (signed) -> out_semantic [2n] int64.
 *   avail (SSR, optional) [n_images] fp64 (the trainer's mask_ids) -> out_avail [1] = avail[image].
 * Indices, form (a) (INERF_BATCH_DRAW clear): image_index (DEVICE, one int64; NULL: the host value image_host), pixels [n]
 *   int64 (q as above), off_row / off_col [n] int64 with values in {-1, 0, 1}.  The library never reads device memory on the
 *   host: a device index outside its table is clamped into it (an offset into [-1, 1]) and INERF_BATCH_STATUS_INDEX is raised.
 * Indices, form (b) (INERF_BATCH_DRAW): drawn in the kernel from (seed, step, ray) by 32-bit integer hashing (no floating point:
 *   tests/_batch_draw.py restates it bit for bit; DESIGN.md section 3, "Training batches").  step is the host value, or *step_dev (one int64) when that is
 *   non-NULL; INERF_BATCH_ADVANCE adds 1 to *step_dev in a second one-thread launch after the batch, so a replayed graph draws a
 *   new batch each time.  Image: hash -> image_ids[j] (DEVICE int64 [n_image_ids]; NULL: j itself, over n_images).  Offsets:
 *   hash -> {-1, 0, 1}.  OBJECT pixels are DISTINCT within a step (np.random.choice(replace=False)): ray k takes perm(k) of a keyed
 *   Feistel bijection on the smallest power-of-two domain covering M = win_h * win_w, cycle-walked back into [0, M).  The walk is
 *   bounded by INERF_BATCH_MAX_WALK; at the bound the value is taken modulo M (a possible duplicate, never a hang) and
 *   INERF_BATCH_STATUS_WALK is raised.  SSR pixels are drawn with replacement (hash mod H*W, as torch.randint).
 *   out_image [1], out_pixels [n], out_off_row [n], out_off_col [n] (int64, optional) receive the indices used, in either form.
 * status: optional device int32 word, OR-ed into (the caller zeroes it).
 * n == 0 is a no-op (INERF_OK, nothing launched, *step_dev untouched).  Returns INERF_E_INVALID for a null required pointer, n < 0,
 * a window that leaves the image, image_host outside [0, n_images), an element size not listed above, n > M in the distinct
 * draw, or INERF_BATCH_ADVANCE without step_dev; INERF_E_UNSUPPORTED for H * W or n beyond 2^31 - 1.  Nothing is allocated,
 * synchronised or read on the host; capturable into a HIP graph.  No atomics except the OR into `status`; bit-identical from run
 * to run and between a direct launch and a replayed one. */
#define INERF_BATCH_OBJECT 0
#define INERF_BATCH_SSR    1
#define INERF_BATCH_DRAW     1u
#define INERF_BATCH_ADVANCE  2u
#define INERF_BATCH_OPENGL   4u
#define INERF_BATCH_STATUS_WALK   1
#define INERF_BATCH_STATUS_INDEX  2
#define INERF_BATCH_MAX_WALK 64
typedef struct inerf_batch_args {
    int32_t form;
    uint32_t flags;
    int64_t n;
    int32_t n_images;
    int32_t height;
    int32_t width;
    int32_t row0;
    int32_t col0;
    int32_t win_h;
    int32_t win_w;
    int32_t pose_stride;
    const float* poses;
    float fx;
    float fy;
    float cx;
    float cy;
    float near;
    float far;
    const float* ray_table;
    const void* images;
    const void* aux;
    const void* semantic;
    const double* avail;
    int32_t image_bytes;
    int32_t aux_bytes;
    int32_t semantic_bytes;
    int32_t image_host;
    const int64_t* image_index;
    const int64_t* pixels;
    const int64_t* off_row;
    const int64_t* off_col;
    uint64_t seed;
    int64_t step;
    int64_t* step_dev;
    const int64_t* image_ids;
    int32_t n_image_ids;
    int32_t reserved;
    float* out_rays;
    void* out_rgb;
    void* out_aux;
    int64_t* out_semantic;
    double* out_avail;
    int64_t* out_image;
    int64_t* out_pixels;
    int64_t* out_off_row;
    int64_t* out_off_col;
    int32_t* status;
} inerf_batch_args;
int inerf_batch_assemble(const inerf_batch_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh extraction: the query lattice of a scene's oriented bounding box and the occupancy of a trained network on it
 * (SSR/extract_colour_mesh.py:149-185, SSR/geometry/occupancy.py:5-48), then marching cubes, the map to scene coordinates, vertex
 * normals and the removal of small components on the device (:186-219: inerf_mc_count, inerf_mc_emit, inerf_mesh_normals,
 * inerf_mesh_clean, further down), then the vertex-colour pass (extract_colour_mesh.py:232-257): one ray per mesh vertex
 * (inerf_vertex_rays), ordinary inerf_render_rays launches, and the 8-bit colour of every vertex written on the device
 * (inerf_vertex_colours), so that three bytes per vertex travel to the host.
 * ------------------------------------------------------------------------------------------- */
#define INERF_MAX_GRID_DIM 1024           /* points per lattice axis: dim^3 <= 2^30 fits the kernels' 32-bit point index */

/* Lattice points [first, first + count) of make_3D_grid (occupancy.py:24-48) as rows of three floats.  Lattice index
 * g = (i * dim + j) * dim + k (torch.meshgrid 'ij': the last axis fastest) lies at
 *   gx = t[i] * scale[0], gy = t[j] * scale[1], gz = t[k] * scale[2]                                        (occupancy.py:34)
 *   out[r] = ((M[r][0] * gx + M[r][1] * gy) + M[r][2] * gz) + M[r][3],  r = 0..2                         (occupancy.py:36-46)
 * every product and every sum rounded to fp32 on its own, in this order: the bits of the reference's CPU tensors
 * (tests/golden/grid_query.npz).  t: [dim] device floats, the axis table - torch.linspace(occ_range[0], occ_range[1], dim)
 * (occupancy.py:25), evaluated by the caller, whose roundings no closed form reproduces (as t_vals of inerf_sample_coarse);
 * scale[3] [host]: extents / (0.9 (occ_range[1] - occ_range[0])) rounded to fp32 (occupancy.py:6-11); transform[12] [host]:
 * rows 0..2 of the box-to-scene matrix, row-major 3 x 4, rounded to fp32 (occupancy.py:9).  Both host arrays travel by value in the
 * kernel arguments.  2 <= dim <= INERF_MAX_GRID_DIM, 0 <= first, first + count <= dim^3, else INERF_E_INVALID; count == 0 is fine. */
int inerf_grid_points(const float* t, int dim, const float* scale /*[host] 3*/, const float* transform /*[host] 12*/,
                      int64_t first, int64_t count, float* out /*[count,3]*/, void* stream);

/* The same function of the same arguments on HOST pointers (t and out included), evaluated by the calling thread: the operation
 * order above can be pinned, and CPU tensors served (geometry.make_3D_grid), without a device. */
int inerf_grid_points_host(const float* t /*[host]*/, int dim, const float* scale /*[host] 3*/, const float* transform /*[host] 12*/,
                           int64_t first, int64_t count, float* out /*[host] [count,3]*/);

/* Occupancy of lattice points [first_point, first_point + n_points) in ONE launch: replaces the chunk loop over run_network, the
 * `.cpu()` after every 1 024 points, raw[..., 3] and occupancy_activation (extract_colour_mesh.py:156-164, 172-179):
 *   sigma = alpha_linear(trunk(embed(x / xyz_div)))  with x = the lattice point as inerf_grid_points gives it
 *   occ_out[i] = 1 - exp(-relu(sigma) * dist)  (a NaN sigma gives NaN, as F.relu does);  sigma_out[i] = sigma  (sigma_out may be NULL)
 * for i = 0 .. n_points - 1.  The density depends on the position alone, so only the position encoding and the eight trunk layers
 * run - neither the direction encoding nor a colour, feature, view or semantic layer - and 4 (8 with sigma_out) bytes per point
 * leave the kernel.  sigma has the bits of channel 3 of inerf_encode_mlp on rays (o = x, d = 0, z = 0): it is the same device code.
 * INERF_PREC_F16X3 only (INERF_E_UNSUPPORTED otherwise; callers evaluate inerf_grid_points through inerf_encode_mlp then), both
 * variants, any class count (the semantic head is not evaluated), l_xyz / l_dir as inerf_encode_mlp.  dim, first_point and
 * n_points as inerf_grid_points.  status: NULL or INERF_STATUS_* words as in inerf_encode_mlp_chunked, here one word per
 * `status_points` LATTICE points - a tile that leaves the f16 range sets word (lattice index / status_points) of every point it
 * holds, so the words cover the whole lattice ([ceil(dim^3 / status_points)]) whatever sub-range a launch takes; status_points == 0:
 * one word.  Null or out-of-range arguments return before anything touches the device. */
int inerf_occupancy_grid(const inerf_net_desc* net, const float* packed_weights, const float* t, int dim,
                         const float* scale /*[host] 3*/, const float* transform /*[host] 12*/, float dist, int64_t first_point,
                         int64_t n_points, float* occ_out /*[n_points]*/, float* sigma_out /*[n_points] or NULL*/,
                         int32_t* status, int64_t status_points, void* stream);

/* element type of inerf_vertex_rays' input rows */
#define INERF_DTYPE_F32 0
#define INERF_DTYPE_F64 1

/* The [n, 11] ray batch of the vertex-colour pass (extract_colour_mesh.py:232-238) in ONE launch: one ray per mesh vertex, cast
 * against the vertex normal from near * near_t in front of the surface.  Per vertex v with normal m, everything in fp32, every
 * operation rounded on its own, nothing contracted - the bits of the reference's CPU tensors (tests/golden/vertex_rays.npz):
 *   d = -m                                                 (:232)   columns 3:6
 *   o_k = v_k - ((d_k * near) * near_t)                    (:235)   columns 0:3; near and near_t are fp32 numbers (what ATen makes
 *                                                                   of `near` = 0.1 * ones and of the Python float args.near_t)
 *   columns 6, 7 = near, far                               (:233-234)
 *   viewdir = d / |d|                                      (:236-237) columns 8:11; the norm and the true division of
 *                                                                   inerf_assemble_rays: |d| = sqrt(fma(d2, d2, fma(d1, d1, d0 * d0)))
 * An all-zero normal gives 0 / 0 = NaN view directions, as the reference does.  It is a source form of inerf_assemble_rays' kernel
 * body (csrc/frame_ops.hip): the view direction and the column writing are that code.
 * vertices / normals: rows of three elements of in_dtype, consecutive rows v_stride / n_stride (>= 3) ELEMENTS apart.
 * INERF_DTYPE_F64 (open3d hands out float64 arrays; the reference rounds them with torch.FloatTensor(...), :232, :235): every
 * element is rounded to the nearest fp32 first, inside the kernel.  rays_out must not overlap the inputs.
 * n == 0 is a no-op, whatever the other arguments.  INERF_E_INVALID: an in_dtype that is neither constant, a null pointer, n < 0, a
 * stride < 3, a pointer not aligned to its element size; INERF_E_UNSUPPORTED beyond (2^31 - 1) * 256 vertices. */
int inerf_vertex_rays(const void* vertices, int64_t v_stride, const void* normals, int64_t n_stride, int64_t n, int in_dtype,
                      float near, float far, float near_t, float* rays_out /*[n,11]*/, void* stream);

/* The same function of the same arguments on HOST pointers, evaluated by the calling thread from the same source
 * (inerf_grid_points_host is its model): the bits can be pinned, and CPU tensors served (geometry.vertex_rays), without a device. */
int inerf_vertex_rays_host(const void* vertices /*[host]*/, int64_t v_stride, const void* normals /*[host]*/, int64_t n_stride,
                           int64_t n, int in_dtype, float near, float far, float near_t, float* rays_out /*[host] [n,11]*/);

/* The 8-bit colour of n mesh vertices from what inerf_render_rays returned for their rays, in ONE launch
 * (extract_colour_mesh.py:248-257).  Exactly one of rgb and logits is non-NULL (both or neither: INERF_E_INVALID):
 *   colour mode (rgb: rows of three floats, rgb_stride >= 3 floats apart): colours_out = to8b(rgb) (:253-255) =
 *     (uint8)(255 * clip(x, 0, 1)), NaN -> 0: byte-equal to inerf_frame_to_u8.  n_classes and colour_map are not read.
 *   semantic mode (logits: rows of n_classes floats, logits_stride >= n_classes floats apart - a column range of a wider row
 *     goes in as it is): label = the label of inerf_sem_maps - its device function, so the lowest index of the row's maximum
 *     logit, and 0 for a row that holds a NaN or whose maximum is not finite - and colours_out = colour_map[label] (:249-251).
 *     colour_map: [n_classes, 3] bytes on the DEVICE (the caller's valid_colour_map).  1 <= n_classes <= INERF_MAX_CLASSES, else
 *     INERF_E_UNSUPPORTED.  labels_out: the labels as int32, or NULL (either mode; not written in colour mode).
 * colours_out: [n, 3] bytes, contiguous.  n == 0 is a no-op once the mode, the strides and n_classes have passed.
 * INERF_E_INVALID: n < 0, a stride smaller than its row, a null colours_out (or colour_map in semantic mode), a float or int32
 * pointer that is not 4-byte aligned; INERF_E_UNSUPPORTED: more than 2^31 - 1 blocks of 256 vertices.  Nothing is allocated,
 * synchronised or read on the host. */
int inerf_vertex_colours(const float* rgb, int64_t rgb_stride, const float* logits, int64_t logits_stride, int64_t n, int n_classes,
                         const unsigned char* colour_map /*[n_classes,3]*/, unsigned char* colours_out /*[n,3]*/,
                         int32_t* labels_out /*[n] or NULL*/, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Marching cubes and mesh cleaning (csrc/mcubes.hip; SSR/extract_colour_mesh.py:186-219): from the occupancy lattice to welded
 * vertices, int32 faces, fp64 vertex normals and a mesh without its small components, all on the device.  The triangulation is this
 * project's own (csrc/mc_tables.h, generated by scripts/gen_mc_tables.py): it is watertight by construction
 * and NOT skimage's Lewiner table, so vertex sets agree with skimage's but faces do not, and degenerate triangles are kept.
 * No kernel waits for another workgroup: every scan is three launches, every atomic is an integer atomic, and the results have
 * the same bytes on every run.  Every entry point checks its arguments before it makes any HIP call.
 *
 * Lattice: occ[nx, ny, nz] floats, the last axis fastest; 2 <= nx, ny, nz (INERF_E_INVALID below) <= INERF_MAX_GRID_DIM and
 * nx * ny * nz <= 2^30 (INERF_E_UNSUPPORTED beyond).  Corner c = di | dj << 1 | dk << 2 of cube (i, j, k) is occ[i + di, j + dj,
 * k + dk]; it is inside iff occ > level (a NaN is outside).  Lattice point (i, j, k) OWNS the up to three lattice edges towards
 * +i, +j and +k; an edge whose ends differ in "inside" carries one vertex.
 * ------------------------------------------------------------------------------------------- */

/* bytes of workspace inerf_mc_count / inerf_mc_emit need for the shape (10 per lattice point and a little); a negative INERF_E_*
 * for a shape outside the limits */
int64_t inerf_mc_workspace_bytes(int nx, int ny, int nz);

/* One tiled pass over the lattice (every value read from memory about once, neighbours through LDS) flags the owned edges of every
 * point and stores the case and triangle count of every cube; two exclusive scans (block sums, one workgroup over the sums, add pass)
 * turn them into vertex and triangle offsets in `workspace`.  totals_dev[3] (int64, device) = {vertices, triangles, non-finite lattice
 * values}: the caller reads it once to size inerf_mc_emit's outputs - the only synchronisation of the stage - and refuses a lattice
 * with non-finite values.  workspace: 256-byte aligned, inerf_mc_workspace_bytes(...) bytes (INERF_E_WORKSPACE if smaller). */
int inerf_mc_count(const float* occ, int nx, int ny, int nz, float level, void* workspace, int64_t workspace_bytes,
                   int64_t* totals_dev /*[3]*/, void* stream);

/* The mesh of the lattice inerf_mc_count just saw (same occ, shape, level and workspace), n_vertices / n_triangles as it reported:
 *   vertices_lattice [n_vertices, 3] floats: in the order owner lattice point (linear index), then axis; on the edge's axis
 *     index + t with t = (level - v0) / (v1 - v0) in plain fp32 (v0 at the owner, v1 at its neighbour), the index elsewhere.
 *     Vertices are welded by construction.  May be NULL when vertices_scene is given.
 *   vertices_scene [n_vertices, 3] doubles, with `affine` [host, 12 doubles: a row-major 3 x 4 map]: row r =
 *     ((A[r][0] x + A[r][1] y) + A[r][2] z) + A[r][3] of the lattice coordinate promoted to double.  Both NULL or both given (not checked for an empty mesh).
 *   faces [n_triangles, 3] int32: in the order cube (linear index of its corner 0), then the table's order; geometric normals
 *     (b - a) x (c - a) point towards lower values - outward for an occupancy, which inerf_vertex_rays relies on.
 * Nothing is written beyond n_vertices rows and n_triangles rows.  INERF_E_UNSUPPORTED: n_vertices > 2^31 - 1 or
 * n_triangles > (2^31 - 1) / 3. */
int inerf_mc_emit(const float* occ, int nx, int ny, int nz, float level, const void* workspace, int64_t workspace_bytes,
                  const double* affine /*[host] 12 or NULL*/, int64_t n_vertices, int64_t n_triangles, float* vertices_lattice,
                  double* vertices_scene, int32_t* faces, void* stream);

/* bytes of workspace inerf_mesh_normals / inerf_mesh_clean need; a negative INERF_E_* for sizes outside the limits above */
int64_t inerf_mesh_workspace_bytes(int64_t n_vertices, int64_t n_triangles);

/* normals_out [n_vertices, 3] doubles: per vertex the fp64 sum, in ASCENDING TRIANGLE INDEX, of the un-normalised cross products
 * (b - a) x (c - a) of its triangles, divided by its length sqrt((x x + y y) + z z); a zero sum stays zero.  open3d's
 * compute_vertex_normals as far as it is known here.  Incident triangles are counted with integer atomics,
 * scanned, filled into slots and sorted per vertex (in registers up to 4 * kMcMaxEdgeTriangles, the most a marching-cubes vertex
 * has), so the bytes do not depend on the run.  A triangle with an index outside [0, n_vertices) contributes nothing. */
int inerf_mesh_normals(const double* vertices /*[n_vertices,3]*/, int64_t n_vertices, const int32_t* faces /*[n_triangles,3]*/,
                       int64_t n_triangles, void* workspace, int64_t workspace_bytes, double* normals_out, void* stream);

/* open3d_utils.clean_mesh (SSR/visualisation/open3d_utils.py:175-201): connected components by lock-free union-find over the
 * vertices (the label of a component is its smallest vertex index), triangles per component by integer atomics, then
 *   keep_single_cluster == 0: triangles of components with fewer than min_triangles triangles are dropped;
 *   keep_single_cluster != 0: only the component with the most triangles stays (a tie: the lowest label); min_triangles is not read;
 * vertices no kept triangle names are dropped.  Both compactions keep the order; faces_out [<= n_triangles, 3] is re-indexed.  Up to
 * three per-vertex arrays of three columns (one float, two double: lattice vertices, scene vertices, normals) are compacted with the
 * same mask: each input NULL with its output, or both given.  Outputs are sized for the input counts and must not overlap inputs.
 * totals_dev[4] (int64, device) = {vertices kept, triangles kept, components that own a triangle, components kept}. */
int inerf_mesh_clean(const int32_t* faces /*[n_triangles,3]*/, int64_t n_vertices, int64_t n_triangles, int64_t min_triangles,
                     int keep_single_cluster, const float* rows_f32, const double* rows_f64_a, const double* rows_f64_b,
                     void* workspace, int64_t workspace_bytes, int32_t* faces_out, float* out_f32, double* out_f64_a,
                     double* out_f64_b, int64_t* totals_dev /*[4]*/, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Validation metrics (csrc/eval.hip): the label and entropy maps of a rendered frame (SSR/training/trainer.py:1244-1245) and the
 * accumulators behind calculate_segmentation_metrics, calculate_depth_metrics and img2mse (SSR/training/training_utils.py:58-124).
 * The host finishing (normalised rows, nanmean, ious, means, square roots) is a few float64 lines on C * C + 14 numbers and stays
 * with the caller (intrinsicnerf_amd/evaluation.py).
 * ------------------------------------------------------------------------------------------- */

/* label[i * label_stride] = the LOWEST index that attains the maximum of logits[i * logits_stride + 0 .. n_classes), as a float;
 * entropy[i * entropy_stride] = -sum_c p_c log p_c of the row's softmax.  Either output may be NULL; each has an element stride
 * of its own, so it can be a column of a frame's pack.
 *   Label: equals the reference's argmax(softmax(x)) whenever the runner-up is bitwise equal to the maximum or below it by more
 *   than fp32 rounding of the softmax can hide; where two logits differ by less than ~1e-7 torch may answer a lower index because
 *   the softmax values round equal - rounding noise of the reference, not reproduced.
 *   A row that holds a NaN, or whose maximum is not finite: label 0, entropy NaN (as torch).  A row with a -inf entry and a finite
 *   maximum: its label, entropy NaN (-(-inf) * 0, as torch).
 *   Entropy: max-subtracted, accurate expf, the two sums and log S - T / S in fp64 (csrc/eval.hip's header comment).
 * 1 <= n_classes <= INERF_MAX_CLASSES, else INERF_E_UNSUPPORTED; n < 0 or a stride smaller than its width (logits_stride <
 * n_classes, an output stride < 1): INERF_E_INVALID.  n == 0 is a no-op.  Nothing is allocated, synchronised or read on the host. */
int inerf_sem_maps(const float* logits, int64_t logits_stride, int64_t n, int n_classes, float* label, int64_t label_stride,
                   float* entropy, int64_t entropy_stride, void* stream);

/* counts[n_classes * n_classes + INERF_EVAL_COUNTS] (int64): the confusion table, row = true label and column = predicted label
 * as sklearn.metrics.confusion_matrix lays it out, then these counters */
#define INERF_EVAL_COUNTS 8
#define INERF_EVAL_N_NOT_IGNORED    0   /* pixels whose true label != ignore_label                       */
#define INERF_EVAL_N_PIXELS         1   /* pixels seen by the depth group                                 */
#define INERF_EVAL_N_PRED_POSITIVE  2   /* ... with depth_pred > 0  ("complete")                         */
#define INERF_EVAL_N_MASK           3   /* ... inside mask = (trgt < 10) * (trgt > 0) * (pred > 0)       */
#define INERF_EVAL_R1               4   /* masked pixels with max(t / p, p / t) < 1.25                    */
#define INERF_EVAL_R2               5   /* ... < 1.5625                                                   */
#define INERF_EVAL_R3               6   /* ... < 1.953125                                                 */
#define INERF_EVAL_N_RGB            7   /* rgb values compared (3 per pixel)                              */
/* sums[INERF_EVAL_SUMS] (double): over the masked pixels, and over every rgb value */
#define INERF_EVAL_SUMS 6
#define INERF_EVAL_ABS_REL      0
#define INERF_EVAL_ABS_DIFF     1
#define INERF_EVAL_SQ_REL       2
#define INERF_EVAL_SQ_DIFF      3
#define INERF_EVAL_SQ_LOG_DIFF  4
#define INERF_EVAL_RGB_SQ       5

/* One pass over n pixels that ADDS into `counts` and `sums`, which the caller owns, zeroes and keeps on the device across frames.
 * Three optional groups:
 *   labels (true_label != NULL): the predicted label is pred_label (a float column) or, when `logits` is non-NULL, derived from
 *     the logits by inerf_sem_maps' device code in this launch - out_label / out_entropy (each optional) are then written as
 *     inerf_sem_maps writes them, also without a true label.  true_label holds floats as the trainer keeps them (label - 1,
 *     void = ignore_label).  A pixel counts as not ignored when true != ignore_label, and enters the table only if, besides, both
 *     labels are integers in [0, n_classes) - a non-integer, a NaN or a label >= n_classes is dropped, as sklearn's labels= does.
 *   depth (depth_pred != NULL, depth_trgt required): training_utils.py:96-109 per pixel in fp32, unfused, in the reference's order:
 *     a = |p - t|, a / t, a * a, (a * a) / t, (logf(p) - logf(t))^2, max(t / p, p / t) against 1.25f, 1.5625f, 1.953125f; with IEEE
 *     division every term but the logarithm has numpy's bits and every count is exact.
 *   rgb (rgb_pred != NULL, rgb_trgt required, 3 floats per pixel `stride` floats apart): (x - y)^2 in fp32 per value.
 * Every stride is in floats.  Bit-identical from run to run: counts through integer atomics (the table privatised in LDS up to 64
 * classes, global beyond), the fp64 sums through fixed trees into one partial row per workgroup in `workspace`
 * (inerf_eval_workspace_bytes(n) bytes, else INERF_E_WORKSPACE) and a second launch that adds the rows in index order.  No
 * floating-point atomic, no hand-off between workgroups inside a kernel; the grid depends on n alone.  Errors as inerf_sem_maps
 * (n_classes is checked whichever groups are given: it sizes `counts`); n == 0 is a no-op; n > 2^31 - 1: INERF_E_UNSUPPORTED.
 * Capturable into a HIP graph. */
typedef struct inerf_eval_args {
    int64_t n;
    int32_t n_classes;
    int32_t ignore_label;
    const float* logits;
    int64_t logits_stride;
    const float* pred_label;
    int64_t pred_label_stride;
    float* out_label;
    int64_t out_label_stride;
    float* out_entropy;
    int64_t out_entropy_stride;
    const float* true_label;
    int64_t true_label_stride;
    const float* depth_pred;
    int64_t depth_pred_stride;
    const float* depth_trgt;
    int64_t depth_trgt_stride;
    const float* rgb_pred;
    int64_t rgb_pred_stride;
    const float* rgb_trgt;
    int64_t rgb_trgt_stride;
    int64_t* counts;
    double* sums;
    void* workspace;
    int64_t workspace_bytes;
} inerf_eval_args;
int64_t inerf_eval_workspace_bytes(int64_t n);
int inerf_eval_accumulate(const inerf_eval_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Intrinsic-image quality metrics (csrc/imq.hip): the sums behind mse / psnr, scale-invariant MSE, LMSE and SSIM / DSSIM of a stack
 * of image pairs.  Neither reference code base has code for these; the definitions below are the contract.
 *   pred, trgt: fp32 [H, W, C], C = 1 or 3.  mask: fp32 [H, W], optional; a pixel is valid iff its mask value > 0 (NaN: invalid);
 *   without a mask every pixel is valid.  M = the number of valid pixels.  Sums run over valid pixels and all channels; products and
 *   sums are fp64 from the fp32 inputs.
 *   mse    = S(g-p)^2 / (C M),  psnr = -10 log10 mse.
 *   si_mse (Grosse et al. 2009 ssq_error; one scale per image, shared by the channels): Spp = S p^2, Spg = S p g, Sgg = S g^2,
 *            a = Spg / Spp if Spp > 1e-5 else 0,  si_mse = S(g - a p)^2 / (C M) = (Sgg - 2 a Spg + a^2 Spp) / (C M).
 *   lmse   (Grosse et al. local_error): k x k windows, k = window_size, at origins i in range(0, H-k+1, s), j in range(0, W-k+1, s),
 *            s = window_shift; each window has its own a_w (same rule, same threshold, over the window's valid pixels);
 *            lmse = sum_w (Sgg_w - 2 a_w Spg_w + a_w^2 Spp_w) / sum_w Sgg_w.  No window or a zero denominator: 0 / 0 = NaN.
 *            1 <= s <= k, k % s == 0 and k / s <= 8, else INERF_E_UNSUPPORTED.
 *   ssim   (Wang et al. 2004, as skimage structural_similarity(gaussian_weights=True, use_sample_covariance=False, data_range=1,
 *            channel_axis=-1)): 11 taps w_i ~ exp(-(i / 1.5)^2 / 2), i = -5..5, normalised in fp64 BY THE CALLER (taps[11]; the
 *            device evaluates no exp); per channel over the (H-10) x (W-10) valid region, no padding: mu_x, mu_y, E[x^2], E[y^2],
 *            E[xy] filtered, sigma^2 and sigma_xy by subtraction,
 *            map = (2 mu_x mu_y + c1)(2 sigma_xy + c2) / ((mu_x^2 + mu_y^2 + c1)(sigma_x^2 + sigma_y^2 + c2)),  c1 = 1e-4, c2 = 9e-4;
 *            ssim = the mean of map over the channels and the positions whose CENTRE pixel is valid (the mask selects positions, it
 *            does not alter what is filtered);  dssim = (1 - ssim) / 2.  H < 11 or W < 11: no position, NaN.
 *   A NaN input propagates to every metric it enters, as in numpy.
 * The host finishing is a few float64 lines on these ten numbers (intrinsicnerf_amd/evaluation.py, finish_image_quality).
 * ------------------------------------------------------------------------------------------- */
/* sums[n_images, INERF_IMQ_SUMS] (double), per image */
#define INERF_IMQ_SUMS 7
#define INERF_IMQ_SPP       0   /* S p^2                                              */
#define INERF_IMQ_SPG       1   /* S p g                                              */
#define INERF_IMQ_SGG       2   /* S g^2                                              */
#define INERF_IMQ_SQ_DIFF   3   /* S (g - p)^2                                        */
#define INERF_IMQ_LMSE_NUM  4   /* sum over windows of S_w (g - a_w p)^2              */
#define INERF_IMQ_LMSE_DEN  5   /* sum over windows of S_w g^2                        */
#define INERF_IMQ_SSIM_SUM  6   /* sum of the SSIM map over channels and positions    */
/* counts[n_images, INERF_IMQ_COUNTS] (int64), per image */
#define INERF_IMQ_COUNTS 3
#define INERF_IMQ_N_VALID   0   /* M: valid pixels (not times C)                      */
#define INERF_IMQ_N_WINDOWS 1   /* LMSE windows                                       */
#define INERF_IMQ_N_SSIM    2   /* SSIM positions with a valid centre (not times C)   */

/* One call for n_images pairs; sums and counts are WRITTEN, not added.  Image i of an input starts i * image_stride floats after
 * the pointer; its pixel (y, x) lies (y * width + x) * pixel_stride floats further and holds `channels` consecutive floats (the
 * mask: one) - so a column range of a frame pack goes in as it is.
 * Four launches: cell moments (the image cut into s x s cells, every pixel read once), windows (each a sum of (k / s)^2 cells),
 * the LDS-tiled separable 11-tap stencil with its halo in LDS, and a one-workgroup-per-image launch that adds the stages' partial
 * rows in index order.  Bit-identical from run to run: no floating-point atomic, fixed fp64 trees into one plain-stored row per
 * workgroup in `workspace` (inerf_image_quality_workspace_bytes(...) bytes, else INERF_E_WORKSPACE); no kernel waits on another
 * workgroup; the grids depend on the shapes alone; nothing is allocated or synchronised; capturable into a HIP graph.
 * INERF_E_INVALID: a NULL args / pred / trgt / sums / counts, a negative size or image stride, a pixel stride smaller than its width
 * (channels; 1 for the mask), a misaligned pointer (4 bytes for floats, 8 for sums / counts / workspace), channels not 1 or 3.
 * INERF_E_UNSUPPORTED: the window rule above, n_images > 65535, height * width > 2^31 - 1.  n_images == 0 or height * width == 0 is
 * a no-op.  inerf_image_quality_workspace_bytes returns the same error codes (negative) for the same arguments. */
typedef struct inerf_imq_args {
    int32_t n_images;
    int32_t height;
    int32_t width;
    int32_t channels;
    const float* pred;
    int64_t pred_pixel_stride;
    int64_t pred_image_stride;
    const float* trgt;
    int64_t trgt_pixel_stride;
    int64_t trgt_image_stride;
    const float* mask;               /* optional */
    int64_t mask_pixel_stride;
    int64_t mask_image_stride;
    int32_t window_size;
    int32_t window_shift;
    double taps[11];
    double c1;
    double c2;
    double* sums;                    /* [n_images, INERF_IMQ_SUMS]   */
    int64_t* counts;                 /* [n_images, INERF_IMQ_COUNTS] */
    void* workspace;
    int64_t workspace_bytes;
} inerf_imq_args;
int64_t inerf_image_quality_workspace_bytes(int64_t n_images, int64_t height, int64_t width, int channels, int window_size,
                                            int window_shift);
int inerf_image_quality(const inerf_imq_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Frame images (csrc/frame_vis.hip): every 8- and 16-bit image the render_path loops write or return, made from the packed frame
 * frame[n, stride] (fp32, a pixel's maps side by side) in one launch - what the reference does on the host per frame: to8b
 * (run_nerf.py:193-211 | trainer.py:1242, 1340-1343, 1379), astype(np.uint16) of disparity and of depth * 1000
 * (trainer.py:1344-1345), the label map's astype(np.uint8) (trainer.py:1318), to8b(acc > 10) (run_nerf.py:173),
 * valid_colour_map[label] (trainer.py:1269, 1294) and imgviz.depth2rgb of depth and entropy (trainer.py:1314, 1321), whose results
 * the trainer stacks, writes as videos and logs (trainer.py:1089-1110, 1394).
 * A PRODUCT reads `width` consecutive columns of the frame from `column` on and writes one plane of bytes, pixel after pixel.
 * All arithmetic is fp32, each operation rounded on its own.  (int32)x below: truncation toward zero, and 0 for NaN or
 * |x| >= 2^31 - what numpy's float32 -> uint16 / uint8 casts give (65535.9 -> 65535, 65536 -> 0, 70000 -> 4464, -1 -> 65535,
 * -0.5 -> 0, NaN, +-inf, 3e9 -> 0).
 *   kind      width   bytes / pixel   rule
 *   TO8B      1 | 3   width           (uint8)(255 * clip(x, 0, 1)), NaN -> 0: byte-equal to inerf_frame_to_u8
 *   U16       1       2, little-endian  the low 16 bits of (int32)(x * a); a = 1: disparity, a = 1000: depth in mm
 *   U8_CAST   1       1               the low 8 bits of (int32)x
 *   THRESH    1       1               x > a ? 255 : 0 (NaN -> 0) = to8b(float32(x > a))
 *   PALETTE   1       3               l = x truncated toward zero; palette[l] (uint8 [n_colours, 3], device) if 0 <= l < n_colours,
 *                                     else (0, 0, 0): NaN, +-inf and |x| >= 2^31 are black too (NOT palette[0], which the
 *                                     (int32) rule's 0 would select), and so is every pixel when n_colours == 0
 *   JET       1       3               t = (x - lo) / (hi - lo); NaN -> (0, 0, 0); else JET[min((int)(clamp(t, 0, 1) * 256), 255)].
 *                                     (lo, hi) = (a, b), or - `range` non-NULL - a device float[2] the kernel reads (the map's
 *                                     own range from inerf_frame_range: no host synchronisation).  hi == lo, +-inf and values
 *                                     outside [lo, hi] have no special case: IEEE arithmetic and the rules above decide
 * JET[256][3] = (matplotlib.colormaps['jet'](arange(256))[:, :3] * 255).round() (csrc/jet_table.h, generated by
 * scripts/gen_jet_table.py; inerf_jet_table() returns its 768 bytes on the host).  With these rules a JET product equals
 * (cmap(where(isnan(t), 0, t))[..., :3] * 255).round().astype(uint8) with black where t is NaN - imgviz.depth2rgb.
 * ------------------------------------------------------------------------------------------- */
#define INERF_FRAME_MAX_PRODUCTS 16
#define INERF_FRAME_TO8B     0
#define INERF_FRAME_U16      1
#define INERF_FRAME_U8_CAST  2
#define INERF_FRAME_THRESH   3
#define INERF_FRAME_PALETTE  4
#define INERF_FRAME_JET      5

typedef struct inerf_frame_product {
    int32_t kind;                    /* INERF_FRAME_* */
    int32_t column;                  /* first column of the frame it reads */
    int32_t width;                   /* columns it reads */
    int32_t reserved;
    float a;                         /* U16: scale; THRESH: threshold; JET: lo */
    float b;                         /* JET: hi */
    const float* range;              /* JET: device float[2] = (lo, hi) read by the kernel instead of (a, b); else NULL */
    int64_t offset;                  /* of its plane in `out`, in bytes: written by inerf_frame_products_layout */
} inerf_frame_product;

typedef struct inerf_frame_products_args {
    const float* frame;              /* [n, stride] fp32, device */
    int64_t stride;                  /* floats between two pixels */
    int64_t n;                       /* pixels */
    int32_t n_products;              /* 0 .. INERF_FRAME_MAX_PRODUCTS */
    int32_t n_colours;
    const unsigned char* palette;    /* [n_colours, 3] uint8, device; read by PALETTE products only */
    unsigned char* out;              /* the planes, device, 16-byte aligned */
    int64_t out_bytes;
    inerf_frame_product products[INERF_FRAME_MAX_PRODUCTS];
} inerf_frame_products_args;

/* Host only, no HIP call: writes products[k].offset - plane k holds n * (bytes / pixel) bytes, pixel after pixel, and starts at a
 * multiple of 16 bytes after plane k - 1 - and returns the byte count `out` needs (0 for n == 0), or a negative error code:
 * INERF_E_INVALID for NULL args, n < 0, n_products outside 0 .. 16, a kind that does not exist or a width its kind does not take. */
int64_t inerf_frame_products_layout(inerf_frame_products_args* args);

/* One launch for all products of one frame.  A workgroup stages the used columns of its 512 pixels in LDS, every column read from
 * memory once however many products use it; a lane takes 4 consecutive pixels and writes whole dwords (4 bytes grey, 8 bytes
 * 16-bit, 12 bytes RGB), the n mod 4 tail byte by byte; the jet table sits in LDS.  No atomics, no hand-off between workgroups,
 * the grid depends on n alone; nothing is allocated, synchronised or read on the host: capturable into a HIP graph.
 * Checked before any HIP call.  INERF_E_INVALID: what inerf_frame_products_layout refuses; offsets that are not the layout's;
 * stride < 1, a product that reads beyond the stride, `range` on a product that is no JET, n_colours < 0; and, for n > 0 and
 * n_products > 0: a NULL frame / out (palette with a PALETTE product and n_colours > 0), out_bytes below the layout's total, a frame or range not
 * 4-byte aligned or an `out` not 16-byte aligned, `out` overlapping the frame, the palette or a range.  INERF_E_UNSUPPORTED:
 * products that read a column beyond the 31st, n beyond 2^31 - 1 workgroups.  n == 0 or n_products == 0 is a no-op. */
int inerf_frame_products(const inerf_frame_products_args* args, void* stream);

/* minmax[0] = nanmin, minmax[1] = nanmax over values[i * stride], i < n, in fp32: NaNs are skipped, +-inf take part, a column
 * that is all NaN gives (NaN, NaN) - a JET product then paints black.  accumulate != 0: the pair minmax holds on entry takes part
 * (the range over a sequence of frames; start it from (NaN, NaN) or from a call with accumulate == 0).  Two launches: one pair per
 * workgroup into `workspace` (inerf_frame_range_workspace_bytes(n) bytes, else INERF_E_WORKSPACE), then one workgroup over the
 * pairs.  No floating-point atomic; a minimum has no order, so the result is the same on every run.  INERF_E_INVALID: n < 0,
 * stride < 1, a NULL or misaligned values / minmax, buffers that overlap.  n == 0 is a no-op (minmax is left as it is). */
int64_t inerf_frame_range_workspace_bytes(int64_t n);
int inerf_frame_range(const float* values, int64_t stride, int64_t n, float* minmax, void* workspace, int64_t workspace_bytes,
                      int accumulate, void* stream);

/* The 768 bytes of JET[256][3] (host memory, static). */
const unsigned char* inerf_jet_table(void);

/* ---------------------------------------------------------------------------------------------
 * PNG files on the device (csrc/png.hip, csrc/png_huff.h): up to 16 image planes - exactly what inerf_frame_products writes, so the
 * encoder chains after that launch with no repacking - become 16 complete PNG files in `dst`, in three launches for all images
 * together.  What render_path otherwise does on the host per file (zlib level 6 over rows of filter type 0).
 * FILE      signature, IHDR, ONE IDAT, IEND, each with its CRC-32.  Colour type 0 (grey, 8 or 16 bit; 16-bit samples big-endian in
 *           the file, little-endian in `src`) or 2 (RGB, 8 bit).  The IDAT is a zlib stream: 0x78 0x01, DEFLATE data, Adler-32.
 * FILTER    per row; INERF_PNG_FILTER_ADAPTIVE takes the type 0 .. 4 with the smallest sum of min(b, 256 - b) over the row's
 *           filtered bytes, ties to the lowest type.  Byte distance 1 (grey 8), 2 (grey 16), 3 (RGB); the row above row 0 is zero.
 * SEGMENT   whole rows, as many as fit 32 768 filtered bytes (1 + width * channels * bit_depth / 8 per row); one workgroup each.
 *           Segments are independent: no match reaches before a segment's first byte.
 * TOKENS    literals and distance-1 matches.  A run of L >= 4 equal bytes is one literal and matches (3 .. 258) over the other
 *           L - 1 bytes: 258s and the remainder; a remainder of 1 or 2 takes bytes from the last 258 and becomes a 3.
 * CODE      one dynamic-Huffman block per segment: HLIT >= 257, HDIST = 1 (one distance code of 1 bit), HCLEN = 19, literal/length
 *           lengths <= 15 and complete, code-length code <= 7 bits and complete, no repeat codes 16 / 17 / 18 in the header.  A
 *           segment whose dynamic block is not smaller than a stored block (5 + bytes) is stored.  Every segment ends on a byte
 *           boundary and is not final - an empty stored block follows a dynamic block that ends inside a byte; one final empty
 *           stored block ends the stream.
 * dst_capacity = 68 + height * (1 + width * channels * bit_depth / 8) + 5 * segments: the stored-everything bound - 8 signature,
 * 25 IHDR, 12 IDAT frame, 2 zlib header, 5 final block, 4 Adler-32, 12 IEND; the filtered bytes; 5 per stored segment.
 * sizes[k] <= dst_capacity always, and no byte of dst outside [dst_offset, dst_offset + dst_capacity) is written.
 * Integer arithmetic only, LDS atomics are integer adds and ORs, no hand-off between workgroups (the stream orders the three
 * launches): the bytes are the same on every run.  Nothing is allocated, synchronised or read on the host: capturable into a HIP
 * graph.
 * ------------------------------------------------------------------------------------------- */
#define INERF_PNG_MAX_IMAGES 16
#define INERF_PNG_FILTER_ADAPTIVE (-1)      /* else 0 .. 4: that PNG filter type on every row */

typedef struct inerf_png_image {
    int32_t height;
    int32_t width;
    int32_t channels;                /* 1 | 3 */
    int32_t bit_depth;               /* 8 | 16; 16 only with channels == 1 */
    int32_t filter;                  /* INERF_PNG_FILTER_ADAPTIVE or 0 .. 4 */
    int32_t reserved;
    int64_t src_offset;              /* of the plane in src, bytes (a product's `offset`); 16-bit planes little-endian */
    int64_t dst_offset;              /* of the file in dst, bytes: written by inerf_png_layout (a multiple of 16) */
    int64_t dst_capacity;            /* written by inerf_png_layout: the worst-case file length, see above */
} inerf_png_image;

typedef struct inerf_png_args {
    const unsigned char* src;        /* the planes, device */
    int64_t src_bytes;
    unsigned char* dst;              /* the files, device, 16-byte aligned */
    int64_t dst_bytes;
    int64_t* sizes;                  /* device int64[n_images]: the length of file k, which starts at dst + images[k].dst_offset */
    void* workspace;                 /* device, 16-byte aligned, inerf_png_workspace_bytes(args) bytes */
    int64_t workspace_bytes;
    int32_t n_images;                /* 0 .. INERF_PNG_MAX_IMAGES */
    int32_t reserved;
    inerf_png_image images[INERF_PNG_MAX_IMAGES];
} inerf_png_args;

/* Host only, no HIP call: writes images[k].dst_offset / dst_capacity and returns the byte count `dst` needs, or a negative error
 * code: INERF_E_INVALID for NULL args, n_images outside 0 .. 16, height or width < 1, channels not 1 | 3, bit_depth not 8 | 16 or
 * 16 with 3 channels, a filter outside -1 .. 4; INERF_E_UNSUPPORTED for a filtered row longer than a segment (32 768 bytes). */
int64_t inerf_png_layout(inerf_png_args* args);

/* Host only: the workspace the call needs (per segment a slot of 32 784 bytes and 32 bytes of bookkeeping), or the layout's error. */
int64_t inerf_png_workspace_bytes(const inerf_png_args* args);

/* Three launches: one workgroup per segment (filter, runs, code, bits; 74 KiB of LDS, two workgroups per CU), one workgroup that
 * scans the segment lengths, combines the segments' Adler-32 sums and CRC-32 registers and writes headers, trailers and sizes, and
 * one workgroup per segment that copies it to its place.  Checked before any HIP call.  INERF_E_INVALID: what inerf_png_layout
 * refuses; dst_offset / dst_capacity that are not the layout's; src_bytes < 0 or a plane that runs past it; and, for n_images > 0:
 * a NULL src / dst / sizes, dst_bytes below the layout's total, dst or workspace not 16-byte aligned, sizes not 8-byte aligned,
 * dst, sizes or workspace overlapping src or each other.  INERF_E_WORKSPACE: a NULL or too small workspace.  n_images == 0 is a
 * no-op. */
int inerf_png_encode(const inerf_png_args* args, void* stream);

/* Host only - the routine of csrc/png_huff.h that the segment kernel runs on one lane: code lengths of a minimum-redundancy prefix
 * code over freq[0 .. n) with no length above `limit`.  A zero count gives length 0; one used symbol length 1; two or more a complete
 * code (Kraft sum 1), the Huffman optimum whenever that fits the limit, else its lengths clamped and repaired (one code leaves the
 * deepest level, one shorter code is split, until the Kraft sum is 1; the longest lengths go to the rarest symbols).  Ties are
 * broken by the symbol index.  INERF_E_INVALID: NULL pointers, n outside 1 .. 288, limit outside 1 .. 15, more used symbols than
 * 2^limit, counts whose sum exceeds 32 bits. */
int inerf_png_code_lengths(const uint32_t* freq, int n, int limit, unsigned char* lengths);

/* ---------------------------------------------------------------------------------------------
 * Frame movies on the device (csrc/jpeg.hip, csrc/jpeg_tables.h): up to 16 image planes - exactly what inerf_frame_products
 * writes - become 16 baseline JPEG files, each appended as one AVI chunk to a device-resident arena: the `movi` payload of a
 * Motion-JPEG AVI file, verbatim.  Replaces imageio.mimwrite / cv2.VideoWriter at the end of the reference's render passes
 * (object_level/run_nerf.py:822, :1051-1052; SSR/training/trainer.py:1088-1093, :1169-1174; gui.py, gui_obj.py,
 * video_generator.py, which names MJPG / .avi as its own alternative container).
 * FILE      SOI, JFIF APP0 (1.01, no units, 1 : 1), DQT (one for grey, two for colour), SOF0 (8 bits; components 1 .. 3, sampling
 *           1 x 1: 4:4:4), DHT (the T.81 Annex K tables: DC then AC, luminance, then chrominance for colour), DRI, SOS, the
 *           entropy-coded data, EOI.  Everything before the data is the HEADER: 334 bytes for grey, 629 for colour, the same for
 *           every frame of a stream; inerf_jpeg_header builds it once on the host and the caller keeps a device copy.
 * TABLES    Annex K luminance / chrominance scaled by quality 1 .. 100 with libjpeg's rule: s = q < 50 ? 5000 / q : 200 - 2 q,
 *           t = clamp((base * s + 50) / 100, 1, 255).  The kernel reads them from the header's DQT segments.
 * SAMPLES   grey: the plane.  Colour: the plane is RGB; Y = (19595 R + 38470 G + 7471 B + 32768) >> 16,
 *           Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16, Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16.
 *           A width or height that is no multiple of 8 repeats the last column / row.
 * DCT       p = sample - 128; M[u][x] = round(8192 a(u) cos((2 x + 1) u pi / 16)), a(0) = sqrt(1 / 8), a(u) = 1 / 2 (tabulated);
 *           rows: t[y][u] = (sum_x M[u][x] p[y][x] + 256) >> 9 (4 fraction bits); columns: c[v][u] = (sum_y M[v][y] t[y][u] + 8192)
 *           >> 14 (3 fraction bits, as libjpeg's coefficients carry), int32, arithmetic shifts.  Quantised:
 *           sign(c) * ((|c| + 4 q) / (8 q)) - round half away from zero of c / (8 q).
 * SEGMENTS  the restart interval is the MCUs of one MCU row: every MCU row starts with predictors 0, is padded to a byte with 1-bits
 *           and followed by RSTm, m = row mod 8, except the last.  One workgroup per (image, MCU row).
 * CHUNK     '00dc', the file's length (little-endian, 4 bytes), the file, one zero byte when that length is odd.
 * ARENA     per image: the arena (device pointer, capacity), a cursor (device int64[2]: bytes used, frames written), an index (device
 *           int64[index_frames][2]: the chunk's offset in the arena and the file's length) and a status word (device int64).  A frame
 *           that fits is appended at the cursor, which advances; images of one call that share an arena land in the call's order.
 *           When a frame does not fit (bytes or index entries), nothing of it is written, the cursor stays and the status word
 *           receives cursor bytes + the chunk's length: the capacity that would have held it.  Nothing else writes the status word.
 * inerf_jpeg_frame_bound = 8 + header + MCU rows * (blocks per row * 416 + 2) + 2 + 1: a block's worst case is 22 + 63 * 26 bits
 * = 208 bytes, every one of them FF and stuffed.  A segment's slot in the workspace has that size.
 * Integer arithmetic only, LDS atomics are ORs, no hand-off between workgroups (the stream orders the three launches): the bytes are
 * the same on every run.  Nothing is allocated, synchronised or read on the host: capturable into a HIP graph, and every replay
 * appends a frame.
 * ------------------------------------------------------------------------------------------- */
#define INERF_JPEG_MAX_IMAGES 16

typedef struct inerf_jpeg_image {
    int32_t height;                  /* 1 .. 65535 */
    int32_t width;                   /* 1 .. 65535 */
    int32_t channels;                /* 1 (grey) | 3 (RGB in the plane, YCbCr 4:4:4 in the file) */
    int32_t quality;                 /* 1 .. 100: what `header` was built with */
    int64_t src_offset;              /* of the plane in src, bytes (a product's `offset`) */
    const unsigned char* header;     /* device: the bytes of inerf_jpeg_header(height, width, channels, quality) */
    int32_t header_bytes;            /* their count: 334 | 629 */
    int32_t reserved;
    unsigned char* arena;            /* device */
    int64_t arena_bytes;             /* its capacity, at least header_bytes */
    int64_t* cursor;                 /* device int64[2], 8-byte aligned: bytes used, frames written */
    int64_t* index;                  /* device int64[index_frames][2], 8-byte aligned: chunk offset, file length */
    int64_t index_frames;            /* >= 1 */
    int64_t* status;                 /* device int64, 8-byte aligned: 0 until a frame did not fit */
} inerf_jpeg_image;

typedef struct inerf_jpeg_args {
    const unsigned char* src;        /* the planes, device */
    int64_t src_bytes;
    void* workspace;                 /* device, 16-byte aligned, inerf_jpeg_workspace_bytes(args) bytes */
    int64_t workspace_bytes;
    int32_t n_images;                /* 0 .. INERF_JPEG_MAX_IMAGES */
    int32_t reserved;
    inerf_jpeg_image images[INERF_JPEG_MAX_IMAGES];
} inerf_jpeg_args;

/* Host only, no HIP call; reads height, width, channels and quality alone: 256 bytes, per segment 16 bytes of bookkeeping and a slot
 * of blocks per row * 416 + 2 bytes (rounded up to 16).  INERF_E_INVALID: NULL args, n_images outside 0 .. 16, a dimension outside
 * 1 .. 65535, channels not 1 | 3, a quality outside 1 .. 100. */
int64_t inerf_jpeg_workspace_bytes(const inerf_jpeg_args* args);

/* Host only: the worst-case chunk length of one frame (see above) - an arena of frames * bound bytes cannot overflow.
 * INERF_E_INVALID as above. */
int64_t inerf_jpeg_frame_bound(int32_t height, int32_t width, int32_t channels);

/* Three launches: one workgroup per segment (transform, quantise, code, stuff; 48 KiB of LDS), one workgroup that sums the segment
 * lengths and reserves the frames' places, one workgroup per segment that copies it to its place.  Checked before any HIP call.
 * INERF_E_INVALID: what inerf_jpeg_workspace_bytes refuses; src_bytes < 0 or a plane that runs past it; a NULL header, arena, cursor,
 * index or status; header_bytes that is not the header's length; arena_bytes < header_bytes; index_frames < 1; cursor, index or
 * status not 8-byte aligned; for n_images > 0 a NULL src or a workspace not 16-byte aligned.  INERF_E_WORKSPACE: a NULL or too small
 * workspace.  n_images == 0 is a no-op. */
int inerf_jpeg_encode(const inerf_jpeg_args* args, void* stream);

/* Host only: the quantisation tables of `quality` in natural (row-major) order, as Pillow's Image.quantization reports them.
 * INERF_E_INVALID: a quality outside 1 .. 100, a NULL pointer. */
int inerf_jpeg_tables(int32_t quality, unsigned char* luma, unsigned char* chroma);

/* Host only: writes the header (see FILE) to dst and returns its length.  INERF_E_INVALID: a bad shape or quality, a NULL dst, a
 * capacity below the header's length. */
int64_t inerf_jpeg_header(int32_t height, int32_t width, int32_t channels, int32_t quality, unsigned char* dst, int64_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* INERF_H */
