"""ctypes binding of the C ABI declared in ``include/inerf.h``.

There is deliberately NO fallback: if ``libinerf.so`` is missing or does not load, importing the
render front-ends raises.  Tensors cross the boundary as raw device pointers (``Tensor.data_ptr()``)
and the current HIP stream handle; torch only owns memory and streams.
"""
import ctypes as C
import os

from . import _build
from ._build import LIB_PATH

ABI_VERSION = 40027         # INERF_ABI_VERSION of include/inerf.h these ctypes declarations mirror

OK, E_INVALID, E_UNSUPPORTED, E_WORKSPACE, E_HIP = 0, -1, -2, -3, -4
VARIANT_OBJECT, VARIANT_SSR = 0, 1
PREC_F32, PREC_F16X3 = 0, 1
STATUS_F16_RANGE = 1
FLAG_WHITE_BKGD, FLAG_LINDISP, FLAG_ENDPOINT, FLAG_U_PER_RAY, FLAG_BINS_DIRECT = 1, 2, 4, 8, 16
FLAG_GATE_COLOUR = 32         # inerf_encode_mlp*: colour heads only on points with positive density (include/inerf.h)
FLAG_GATE_PROBE = 64          # ... with a one-product probe of the trunk in front: only its candidates take the exact trunk
CLUSTER_IGNORE_LABEL = 1
CAM_OPENGL = 1
BASE_CHANNELS, ENDPOINT_DIM, RAY_FLOATS, MAX_CLASSES = 11, 128, 11, 240
# size limits of the per-ray stage kernels (INERF_MAX_SAMPLES ... of include/inerf.h): E_UNSUPPORTED beyond them
MAX_SAMPLES, MIN_COARSE, MAX_COARSE, MIN_BINS, MAX_IMPORTANCE = 1024, 3, 256, 2, 512
MAX_GRID_DIM = 1024           # INERF_MAX_GRID_DIM: points per axis of the mesh-extraction lattice
DTYPE_F32, DTYPE_F64 = 0, 1   # INERF_DTYPE_*: element type of inerf_vertex_rays' vertex and normal rows

_ERR = {E_INVALID: "invalid argument", E_UNSUPPORTED: "unsupported configuration",
        E_WORKSPACE: "workspace missing or too small", E_HIP: "HIP runtime error"}


class NetDesc(C.Structure):
    _fields_ = [("variant", C.c_int32), ("n_classes", C.c_int32), ("l_xyz", C.c_int32), ("l_dir", C.c_int32),
                ("xyz_div", C.c_float), ("precision", C.c_int32)]


class CompositeOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in
                ("rgb", "disp", "acc", "depth", "albedo", "shading", "residual", "sem", "feat", "weights")]


class RenderArgs(C.Structure):
    _fields_ = [("net", NetDesc), ("packed_coarse", C.c_void_p), ("packed_fine", C.c_void_p),
                ("rays", C.c_void_p), ("n_rays", C.c_int64), ("n_samples", C.c_int32), ("n_importance", C.c_int32),
                ("flags", C.c_uint32), ("t_vals", C.c_void_p), ("t_rand", C.c_void_p), ("u", C.c_void_p),
                ("noise_coarse", C.c_void_p), ("noise_fine", C.c_void_p),
                ("coarse", CompositeOut), ("fine", CompositeOut), ("z_std", C.c_void_p),
                ("raw_coarse", C.c_void_p), ("raw_fine", C.c_void_p), ("z_coarse", C.c_void_p),
                ("z_samples", C.c_void_p), ("z_fine", C.c_void_p), ("status", C.c_void_p), ("status_rays", C.c_int64),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("gate_state_coarse", C.c_void_p), ("gate_state_fine", C.c_void_p)]


class LinearArgs(C.Structure):
    _fields_ = [("a", C.c_void_p), ("a_sm", C.c_int64), ("a_sk", C.c_int64), ("b", C.c_void_p), ("b_sn", C.c_int64), ("b_sk", C.c_int64),
                ("bias", C.c_void_p), ("add", C.c_void_p), ("add_ld", C.c_int64), ("gate", C.c_void_p), ("gate_ld", C.c_int64),
                ("c", C.c_void_p), ("c_ld", C.c_int64), ("m", C.c_int64), ("n", C.c_int32), ("act", C.c_int32), ("k", C.c_int64)]


ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2


class ClusterFitArgs(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("labels", C.c_void_p), ("n_pixels", C.c_int64), ("n_classes", C.c_int32),
                ("max_class_samples", C.c_int32), ("sample_idx", C.c_void_p), ("sample_begin", C.c_void_p),
                ("n_sample_idx", C.c_int64), ("factor", C.c_void_p), ("quantile", C.c_double), ("band_factor", C.c_double),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("out_bandwidth", C.c_void_p),
                ("out_centers", C.c_void_p), ("out_center_begin", C.c_void_p), ("out_anchors", C.c_void_p),
                ("out_links", C.c_void_p), ("out_anchor_begin", C.c_void_p), ("out_mapped_centers", C.c_void_p),
                ("out_center_counts", C.c_void_p), ("out_pixel_label", C.c_void_p), ("out_class_stats", C.c_void_p),
                ("status", C.c_void_p)]


class LossLevel(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("albedo", "shading", "residual", "rgb", "logits",
                                          "d_albedo", "d_shading", "d_residual", "d_rgb", "d_logits")]


class LossArgs(C.Structure):
    _fields_ = [("n_rays", C.c_int64), ("n_levels", C.c_int32), ("n_classes", C.c_int32), ("flags", C.c_uint32),
                ("ce_label_offset", C.c_int32), ("gt_rgb", C.c_void_p), ("pair_key", C.c_void_p), ("cluster_target", C.c_void_p),
                ("ce_labels", C.c_void_p), ("weights", C.c_void_p), ("grad_total", C.c_void_p), ("grad_terms", C.c_void_p),
                ("level", LossLevel * 2), ("state", C.c_void_p), ("state_bytes", C.c_int64)]


class AdamArgs(C.Structure):
    _fields_ = [("n_tensors", C.c_int32), ("params", C.c_void_p), ("grads", C.c_void_p), ("exp_avg", C.c_void_p),
                ("exp_avg_sq", C.c_void_p), ("steps", C.c_void_p), ("counts", C.c_void_p), ("lr", C.c_float),
                ("lr_dev", C.c_void_p), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double)]


class BatchArgs(C.Structure):
    _fields_ = [("form", C.c_int32), ("flags", C.c_uint32), ("n", C.c_int64), ("n_images", C.c_int32), ("height", C.c_int32),
                ("width", C.c_int32), ("row0", C.c_int32), ("col0", C.c_int32), ("win_h", C.c_int32), ("win_w", C.c_int32),
                ("pose_stride", C.c_int32), ("poses", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("near", C.c_float), ("far", C.c_float), ("ray_table", C.c_void_p), ("images", C.c_void_p),
                ("aux", C.c_void_p), ("semantic", C.c_void_p), ("avail", C.c_void_p), ("image_bytes", C.c_int32),
                ("aux_bytes", C.c_int32), ("semantic_bytes", C.c_int32), ("image_host", C.c_int32), ("image_index", C.c_void_p),
                ("pixels", C.c_void_p), ("off_row", C.c_void_p), ("off_col", C.c_void_p), ("seed", C.c_uint64), ("step", C.c_int64),
                ("step_dev", C.c_void_p), ("image_ids", C.c_void_p), ("n_image_ids", C.c_int32), ("reserved", C.c_int32),
                ("out_rays", C.c_void_p), ("out_rgb", C.c_void_p), ("out_aux", C.c_void_p), ("out_semantic", C.c_void_p),
                ("out_avail", C.c_void_p), ("out_image", C.c_void_p), ("out_pixels", C.c_void_p), ("out_off_row", C.c_void_p),
                ("out_off_col", C.c_void_p), ("status", C.c_void_p)]


BATCH_OBJECT, BATCH_SSR = 0, 1
BATCH_DRAW, BATCH_ADVANCE, BATCH_OPENGL = 1, 2, 4
BATCH_STATUS_WALK, BATCH_STATUS_INDEX = 1, 2
BATCH_MAX_WALK = 64

class DrawArgs(C.Structure):
    """inerf_draw_args: the training draws (include/inerf.h, "Training draws")."""
    _fields_ = [("seed", C.c_uint64), ("step", C.c_int64), ("step_dev", C.c_void_p), ("ray_base", C.c_uint64),
                ("noise_std", C.c_float), ("flags", C.c_uint32)]


class EditParams(C.Structure):
    """inerf_edit_params: the edit state of the scene-editing kernels (include/inerf.h, inerf_edit_frame)."""
    _fields_ = [("edit_centers", C.c_void_p), ("shading_mode", C.c_int32), ("residual_mode", C.c_int32),
                ("shading_scale", C.c_float), ("residual_scale", C.c_float)]


class Ndc(C.Structure):
    """inerf_ndc: the NDC projection's coefficients (include/inerf.h, inerf_gen_rays_ndc)."""
    _fields_ = [("sx", C.c_float), ("sy", C.c_float), ("near_plane", C.c_float)]


class EvalArgs(C.Structure):
    """inerf_eval_args: one accumulate pass of the validation metrics (include/inerf.h, inerf_eval_accumulate)."""
    _fields_ = [("n", C.c_int64), ("n_classes", C.c_int32), ("ignore_label", C.c_int32),
                ("logits", C.c_void_p), ("logits_stride", C.c_int64), ("pred_label", C.c_void_p), ("pred_label_stride", C.c_int64),
                ("out_label", C.c_void_p), ("out_label_stride", C.c_int64), ("out_entropy", C.c_void_p), ("out_entropy_stride", C.c_int64),
                ("true_label", C.c_void_p), ("true_label_stride", C.c_int64), ("depth_pred", C.c_void_p), ("depth_pred_stride", C.c_int64),
                ("depth_trgt", C.c_void_p), ("depth_trgt_stride", C.c_int64), ("rgb_pred", C.c_void_p), ("rgb_pred_stride", C.c_int64),
                ("rgb_trgt", C.c_void_p), ("rgb_trgt_stride", C.c_int64), ("counts", C.c_void_p), ("sums", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


EVAL_COUNTS, EVAL_SUMS = 8, 6
EVAL_COUNT_NAMES = ("n_not_ignored", "n_pixels", "n_pred_positive", "n_mask", "r1", "r2", "r3", "n_rgb")
EVAL_SUM_NAMES = ("abs_rel", "abs_diff", "sq_rel", "sq_diff", "sq_log_diff", "rgb_sq")



class ImqArgs(C.Structure):
    """inerf_imq_args: one image-quality call over a stack of image pairs (include/inerf.h, inerf_image_quality)."""
    _fields_ = [("n_images", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("pred", C.c_void_p), ("pred_pixel_stride", C.c_int64), ("pred_image_stride", C.c_int64),
                ("trgt", C.c_void_p), ("trgt_pixel_stride", C.c_int64), ("trgt_image_stride", C.c_int64),
                ("mask", C.c_void_p), ("mask_pixel_stride", C.c_int64), ("mask_image_stride", C.c_int64),
                ("window_size", C.c_int32), ("window_shift", C.c_int32), ("taps", C.c_double * 11), ("c1", C.c_double), ("c2", C.c_double),
                ("sums", C.c_void_p), ("counts", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


IMQ_SUMS, IMQ_COUNTS = 7, 3
IMQ_SUM_NAMES = ("spp", "spg", "sgg", "sq_diff", "lmse_num", "lmse_den", "ssim_sum")
IMQ_COUNT_NAMES = ("n_valid", "n_windows", "n_ssim")


class FrameProduct(C.Structure):
    """inerf_frame_product: one image plane made from columns of a packed frame (include/inerf.h, inerf_frame_products)."""
    _fields_ = [("kind", C.c_int32), ("column", C.c_int32), ("width", C.c_int32), ("reserved", C.c_int32), ("a", C.c_float),
                ("b", C.c_float), ("range", C.c_void_p), ("offset", C.c_int64)]


FRAME_MAX_PRODUCTS = 16
FRAME_TO8B, FRAME_U16, FRAME_U8_CAST, FRAME_THRESH, FRAME_PALETTE, FRAME_JET = range(6)
FRAME_KIND_NAMES = ("to8b", "u16", "u8_cast", "thresh", "palette", "jet")
FRAME_BYTES_PER_PIXEL = {FRAME_U16: 2, FRAME_U8_CAST: 1, FRAME_THRESH: 1, FRAME_PALETTE: 3, FRAME_JET: 3}      # TO8B: its width


class FrameProductsArgs(C.Structure):
    """inerf_frame_products_args: all image planes of one frame in one launch (include/inerf.h, inerf_frame_products)."""
    _fields_ = [("frame", C.c_void_p), ("stride", C.c_int64), ("n", C.c_int64), ("n_products", C.c_int32), ("n_colours", C.c_int32),
                ("palette", C.c_void_p), ("out", C.c_void_p), ("out_bytes", C.c_int64), ("products", FrameProduct * FRAME_MAX_PRODUCTS)]


class PngImage(C.Structure):
    """inerf_png_image: one plane to encode and where its file goes (include/inerf.h, inerf_png_encode)."""
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32), ("bit_depth", C.c_int32), ("filter", C.c_int32),
                ("reserved", C.c_int32), ("src_offset", C.c_int64), ("dst_offset", C.c_int64), ("dst_capacity", C.c_int64)]


PNG_MAX_IMAGES = 16
PNG_FILTER_ADAPTIVE = -1
PNG_SEGMENT_BYTES = 32768      # filtered bytes per segment (csrc/png.hip)


class PngArgs(C.Structure):
    """inerf_png_args: up to 16 planes -> 16 PNG files in three launches (include/inerf.h, inerf_png_encode)."""
    _fields_ = [("src", C.c_void_p), ("src_bytes", C.c_int64), ("dst", C.c_void_p), ("dst_bytes", C.c_int64), ("sizes", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("n_images", C.c_int32), ("reserved", C.c_int32),
                ("images", PngImage * PNG_MAX_IMAGES)]


class JpegImage(C.Structure):
    """inerf_jpeg_image: one plane to encode and the stream (header, arena, cursor, index, status) its frame is appended to
    (include/inerf.h, inerf_jpeg_encode)."""
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32), ("quality", C.c_int32), ("src_offset", C.c_int64),
                ("header", C.c_void_p), ("header_bytes", C.c_int32), ("reserved", C.c_int32), ("arena", C.c_void_p),
                ("arena_bytes", C.c_int64), ("cursor", C.c_void_p), ("index", C.c_void_p), ("index_frames", C.c_int64),
                ("status", C.c_void_p)]


JPEG_MAX_IMAGES = 16


class JpegArgs(C.Structure):
    """inerf_jpeg_args: up to 16 planes -> 16 JPEG files in AVI chunks in three launches (include/inerf.h, inerf_jpeg_encode)."""
    _fields_ = [("src", C.c_void_p), ("src_bytes", C.c_int64), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("n_images", C.c_int32), ("reserved", C.c_int32), ("images", JpegImage * JPEG_MAX_IMAGES)]


DRAW_STREAM_JITTER, DRAW_STREAM_NOISE_COARSE, DRAW_STREAM_U, DRAW_STREAM_NOISE_FINE = 0, 1, 2, 3
DRAW_PERTURB, DRAW_FINE = 1, 2

ADAM_TABLE_TENSORS = 72      # tensors per launch of inerf_adam_step (its by-value kernel-argument table)

LOSS_KEY_LABELS, LOSS_MASK_OUTER = 1, 2
LOSS_TERMS, LOSS_STATE_FLOATS, LOSS_MAX_CLASSES = 9, 16, 101
LOSS_TERM_NAMES = ("chroma", "residual", "sparsity", "shading", "far", "intensity", "image", "cluster", "semantic")

CLUSTER_FIT_NONFINITE, CLUSTER_FIT_RANGE, CLUSTER_FIT_SAMPLE = 1, 2, 4

# every symbol include/inerf.h declares: (restype, argtypes)
_P, _I, _L, _U = C.c_void_p, C.c_int, C.c_int64, C.c_uint32
SYMBOLS = {
    "inerf_version": (C.c_char_p, []),
    "inerf_abi_version": (_I, []),
    "inerf_build_digest": (C.c_char_p, []),
    "inerf_last_hip_error": (_I, []),
    "inerf_num_tensors": (_I, [C.POINTER(NetDesc)]),
    "inerf_tensor_info": (_I, [C.POINTER(NetDesc), _I, C.POINTER(C.c_char_p), C.POINTER(_L), C.POINTER(_L)]),
    "inerf_packed_floats": (_L, [C.POINTER(NetDesc)]),
    "inerf_raw_channels": (_I, [C.POINTER(NetDesc), _U, _I]),
    "inerf_pack_weights": (_I, [C.POINTER(NetDesc), C.POINTER(_P), _I, _P, _L]),
    "inerf_sample_coarse": (_I, [_P, _P, _P, _L, _I, _U, _P, _P]),
    "inerf_encode_mlp": (_I, [C.POINTER(NetDesc), _P, _P, _P, _L, _I, _U, _P, _P, _P]),
    "inerf_encode_mlp_workspace_bytes": (_L, [C.POINTER(NetDesc), _L, _I, _U]),
    "inerf_encode_mlp_ws": (_I, [C.POINTER(NetDesc), _P, _P, _P, _L, _I, _U, _P, _P, _P, _L, _P]),
    "inerf_encode_mlp_chunked": (_I, [C.POINTER(NetDesc), _P, _P, _P, _L, _I, _U, _P, _P, _L, _P, _L, _P]),
    "inerf_encode_mlp_probed": (_I, [C.POINTER(NetDesc), _P, _P, _P, _L, _I, _U, _P, _P, _L, _P, _L, _P, _P]),
    "inerf_encode_mlp_margin": (_I, [C.POINTER(NetDesc), _P, _P, _P, _L, _I, _U, _P, _P, _L, _P, _L, _P, _P, _P]),
    "inerf_gate_kappa": (C.c_float, [C.c_float, _L, _L]),
    "inerf_gate_min_observed": (_L, []),
    "inerf_mlp_save_floats": (_L, [C.POINTER(NetDesc), _L]),
    "inerf_mlp_save_slot": (_I, [C.POINTER(NetDesc), _I, _L, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "inerf_encode_mlp_train": (_I, [C.POINTER(NetDesc), _P, _P, _P, _L, _I, _U, _P, _P, _P, _P, _P]),
    "inerf_bwd_packed_floats": (_L, [C.POINTER(NetDesc)]),
    "inerf_pack_weights_bwd": (_I, [C.POINTER(NetDesc), C.POINTER(_P), _I, _P, _L]),
    "inerf_mlp_backward_inputs": (_I, [C.POINTER(NetDesc), _P, _P, _P, _P, _L, _U, _P, _P, _P, _P, _P]),
    "inerf_mlp_head_partial_floats": (_I, []),
    "inerf_mlp_backward_grid": (_I, [_L]),
    "inerf_wgrad_grid": (_I, [_L]),
    "inerf_mlp_weight_gradient": (_I, [_P, _I, _P, _I, _L, _I, _I, _P, _P, _P, _L, _P]),
    "inerf_mlp_weight_gradient_gfrag": (_I, [_P, _P, _P, _I, _L, _I, _P, _P, _P, _L, _P]),
    "inerf_mlp_weight_gradient_xfrag": (_I, [_P, _I, _P, _L, _I, _P, _P, _P, _L, _P]),
    "inerf_wgrad_frag_grid": (_I, [_L, _I]),
    "inerf_wgrad_frag_rows": (_I, [_L, _I, C.POINTER(C.c_int), C.POINTER(C.c_int), _I]),
    "inerf_mlp_weight_gradient_frag_batch": (_I, [_I, C.POINTER(_P), _P, C.POINTER(_P), C.POINTER(C.c_int), C.POINTER(C.c_int), _P, _L, C.POINTER(_P),
                                                  C.POINTER(_P), _L, _P]),
    "inerf_mlp_weight_gradient_frag": (_I, [_P, _P, _P, _P, _L, _P, _P, _L, _P]),
    "inerf_mlp_save_slot_is_fragment": (_I, [_I, _I]),
    "inerf_param_floats": (_L, [C.POINTER(NetDesc)]),
    "inerf_mlp_backward_workspace_bytes": (_L, [C.POINTER(NetDesc), _L]),
    "inerf_mlp_backward": (_I, [C.POINTER(NetDesc), _P, _P, _P, _P, _P, _L, _U, _P, _P, _L, _P, _P]),
    "inerf_pack_map": (_L, [C.POINTER(NetDesc), _I, _P, _P, _L, _P, _P, _P, _P, _P, _L, C.POINTER(C.c_int32)]),
    "inerf_repack": (_I, [C.POINTER(_P), C.POINTER(_L), _I, _P, _P, _L, _P, _I, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P]),
    "inerf_composite": (_I, [_P, _P, _P, _I, _P, _L, _I, _I, _I, _I, _U, C.POINTER(CompositeOut), _P]),
    "inerf_composite_backward": (_I, [_P, _P, _P, _I, _P, _L, _I, _I, _I, _I, _U, C.POINTER(CompositeOut), _P, _P]),
    "inerf_sample_fine": (_I, [_P, _P, _P, _L, _I, _I, _U, _P, _P, _P, _P]),
    "inerf_sample_pdf": (_I, [_P, _P, _P, _L, _I, _I, _U, _P, _P]),
    "inerf_workspace_bytes": (_L, [C.POINTER(NetDesc), _L, _I, _I, _U]),
    "inerf_render_workspace_bytes": (_L, [C.POINTER(RenderArgs)]),
    "inerf_render_rays": (_I, [C.POINTER(RenderArgs), _P]),
    "inerf_gen_rays": (_I, [_P, _I, _P, _I, _I, _I, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _U, _P, _P]),
    "inerf_gen_rays_ndc": (_I, [_P, _I, _P, _I, _I, _I, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _U,
                                C.POINTER(Ndc), _P, _P]),
    "inerf_assemble_rays": (_I, [_P, _L, _P, _L, _L, C.c_float, C.c_float, C.POINTER(Ndc), _P, _P]),
    "inerf_ndc_rays": (_I, [_P, _L, _P, _L, _L, C.POINTER(Ndc), _P, _P, _P]),
    "inerf_frame_to_u8": (_I, [_P, _L, _P, _P]),
    "inerf_cluster_lookup": (_I, [_P, _P, _L, _P, _P, _P, _P, _P, _P, _I, _U, _P, _P, _P]),
    "inerf_cluster_fit_workspace_bytes": (_L, [_L, _I, _L]),
    "inerf_cluster_fit": (_I, [C.POINTER(ClusterFitArgs), _P]),
    "inerf_frame_subsample": (_I, [_P, _L, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P]),
    "inerf_cluster_snap_compose": (_I, [_P, _P, _P, _P, _L, _L, _P, _P, _P, _P, _P, _P, _I, _U, _P, _P, _P, _P]),
    "inerf_edit_frame": (_I, [_P, _P, _P, _P, _L, _L, _P, _P, _P, _P, _P, _I, _U, C.POINTER(EditParams), _P, _P, _P, _P, _P]),
    "inerf_edit_recompose": (_I, [_P, _P, _P, _L, _P, _L, C.POINTER(EditParams), _P, _P, _P, _P]),
    "inerf_edit_recompose_u8": (_I, [_P, _P, _P, _P, _L, C.POINTER(EditParams), _P, _P, _P, _P]),
    "inerf_linear": (_I, [C.POINTER(LinearArgs), _P]),
    "inerf_linear_wgrad_workspace_bytes": (_L, [_L, _I, _I]),
    "inerf_linear_wgrad": (_I, [_P, _L, _I, _P, _L, _I, _L, _P, _P, _I, _P, _L, _P]),
    "inerf_embed": (_I, [_P, _P, _L, _I, _I, C.c_float, _I, _P, _L, _P]),
    "inerf_intrinsic_combine": (_I, [_P, _L, _L, _P]),
    "inerf_intrinsic_combine_backward": (_I, [_P, _P, _L, _L, _P, _P]),
    "inerf_intrinsic_loss_workspace_bytes": (_L, [_L, _I]),
    "inerf_intrinsic_loss": (_I, [C.POINTER(LossArgs), _P]),
    "inerf_intrinsic_loss_backward": (_I, [C.POINTER(LossArgs), _P]),
    "inerf_adam_step": (_I, [C.POINTER(AdamArgs), _P]),
    "inerf_batch_assemble": (_I, [C.POINTER(BatchArgs), _P]),
    "inerf_draw_fill": (_I, [C.POINTER(DrawArgs), _I, _L, _I, _P, _P]),
    "inerf_draw_advance": (_I, [_P, _P]),
    "inerf_sample_coarse_drawn": (_I, [_P, _P, _P, _L, _I, _U, _P, C.POINTER(DrawArgs), _P]),
    "inerf_composite_drawn": (_I, [_P, _P, _P, _I, _P, _L, _I, _I, _I, _I, _U, C.POINTER(CompositeOut), C.POINTER(DrawArgs), _P]),
    "inerf_composite_backward_drawn": (_I, [_P, _P, _P, _I, _P, _L, _I, _I, _I, _I, _U, C.POINTER(CompositeOut), _P,
                                            C.POINTER(DrawArgs), _P]),
    "inerf_sample_fine_drawn": (_I, [_P, _P, _P, _L, _I, _I, _U, _P, _P, _P, C.POINTER(DrawArgs), _P]),
    "inerf_sample_pdf_drawn": (_I, [_P, _P, _P, _L, _I, _I, _U, _P, C.POINTER(DrawArgs), _P]),
    "inerf_render_rays_drawn": (_I, [C.POINTER(RenderArgs), C.POINTER(DrawArgs), _P]),
    "inerf_grid_points": (_I, [_P, _I, C.POINTER(C.c_float), C.POINTER(C.c_float), _L, _L, _P, _P]),
    "inerf_grid_points_host": (_I, [_P, _I, C.POINTER(C.c_float), C.POINTER(C.c_float), _L, _L, _P]),
    "inerf_occupancy_grid": (_I, [C.POINTER(NetDesc), _P, _P, _I, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, _L, _L, _P, _P, _P, _L, _P]),
    "inerf_vertex_rays": (_I, [_P, _L, _P, _L, _L, _I, C.c_float, C.c_float, C.c_float, _P, _P]),
    "inerf_vertex_rays_host": (_I, [_P, _L, _P, _L, _L, _I, C.c_float, C.c_float, C.c_float, _P]),
    "inerf_vertex_colours": (_I, [_P, _L, _P, _L, _L, _I, _P, _P, _P, _P]),
    "inerf_mc_workspace_bytes": (_L, [_I, _I, _I]),
    "inerf_mc_count": (_I, [_P, _I, _I, _I, C.c_float, _P, _L, _P, _P]),
    "inerf_mc_emit": (_I, [_P, _I, _I, _I, C.c_float, _P, _L, C.POINTER(C.c_double), _L, _L, _P, _P, _P, _P]),
    "inerf_mesh_workspace_bytes": (_L, [_L, _L]),
    "inerf_mesh_normals": (_I, [_P, _L, _P, _L, _P, _L, _P, _P]),
    "inerf_mesh_clean": (_I, [_P, _L, _L, _L, _I, _P, _P, _P, _P, _L, _P, _P, _P, _P, _P, _P]),
    "inerf_sem_maps": (_I, [_P, _L, _L, _I, _P, _L, _P, _L, _P]),
    "inerf_eval_workspace_bytes": (_L, [_L]),
    "inerf_eval_accumulate": (_I, [C.POINTER(EvalArgs), _P]),
    "inerf_image_quality_workspace_bytes": (_L, [_L, _L, _L, _I, _I, _I]),
    "inerf_image_quality": (_I, [C.POINTER(ImqArgs), _P]),
    "inerf_frame_products_layout": (_L, [C.POINTER(FrameProductsArgs)]),
    "inerf_frame_products": (_I, [C.POINTER(FrameProductsArgs), _P]),
    "inerf_frame_range_workspace_bytes": (_L, [_L]),
    "inerf_frame_range": (_I, [_P, _L, _L, _P, _P, _L, _I, _P]),
    "inerf_jet_table": (C.POINTER(C.c_ubyte * 768), []),
    "inerf_png_layout": (_L, [C.POINTER(PngArgs)]),
    "inerf_png_workspace_bytes": (_L, [C.POINTER(PngArgs)]),
    "inerf_png_encode": (_I, [C.POINTER(PngArgs), _P]),
    "inerf_png_code_lengths": (_I, [C.POINTER(C.c_uint32), _I, _I, C.POINTER(C.c_ubyte)]),
    "inerf_jpeg_workspace_bytes": (_L, [C.POINTER(JpegArgs)]),
    "inerf_jpeg_frame_bound": (_L, [C.c_int32, C.c_int32, C.c_int32]),
    "inerf_jpeg_encode": (_I, [C.POINTER(JpegArgs), _P]),
    "inerf_jpeg_tables": (_I, [C.c_int32, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "inerf_jpeg_header": (_L, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_ubyte), _L]),
}

_lib = None


def lib():
    """The loaded library (loads on first use; raises if it is not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH) and "INERF_LIB_OVERRIDE" not in os.environ and not _build.have_hipcc():
            raise RuntimeError(
                f"{LIB_PATH} is not built.  Run `python -c 'import __graft_entry__ as g; g.build()'` (or "
                "`python -m intrinsicnerf_amd._build`).  intrinsicnerf_amd has no CPU or eager fallback.")
        path = os.environ.get("INERF_LIB_OVERRIDE", LIB_PATH)               # kernel-tuning experiments load variant builds
        if path == LIB_PATH and _build._stale():
            # the library was built from other sources, headers or flags than the tree holds (content digest linked into
            # it, _build.source_digest): the hand-mirrored structs below may no longer match it.  Rebuild when the
            # toolchain is here, refuse to load otherwise - never run a stale library.
            if _build.have_hipcc():
                _build.build_library()
            else:
                raise RuntimeError(f"{LIB_PATH} was built from different sources (digest {_build.built_digest()[:12]}, tree "
                                   f"{_build.source_digest()[:12]}) and hipcc is not available to rebuild it")
        if path != LIB_PATH and _build.sources_present() and _build.built_digest(path) != _build.source_digest():
            # an override library is loaded as asked for (the ABI number below is its only guard) - but never silently
            import warnings
            warnings.warn(f"INERF_LIB_OVERRIDE={path}: built from other sources than this tree (digest "
                          f"{_build.built_digest(path)[:12] or 'none'}, tree {_build.source_digest()[:12]})")
        handle = C.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(handle, name)          # AttributeError here = header/library mismatch
            fn.restype, fn.argtypes = res, args
        got = handle.inerf_abi_version()
        if got != ABI_VERSION:
            raise RuntimeError(f"{path} reports ABI {got}, this binding was written for {ABI_VERSION}: rebuild the "
                               "library (python -m intrinsicnerf_amd._build) or update _capi.py")
        _lib = handle
    return _lib


def check(rc, what):
    if rc == OK:
        return
    msg = _ERR.get(rc, f"error {rc}")
    if rc == E_HIP:
        msg += f" (hipError_t {lib().inerf_last_hip_error()})"
    raise RuntimeError(f"{what}: {msg}")


_forced_precision = None


class forced_precision:
    """Context manager: every ``default_precision()`` inside answers ``prec`` (used to re-render a whole frame with the
    exact fp32 kernel after the split-precision one reported an out-of-range activation)."""

    def __init__(self, prec):
        self.prec = prec

    def __enter__(self):
        global _forced_precision
        self.saved, _forced_precision = _forced_precision, self.prec

    def __exit__(self, *exc):
        global _forced_precision
        _forced_precision = self.saved


def default_precision():
    """MLP arithmetic used when a caller does not choose: $INERF_PRECISION = f16x3 (default) | f32.

    f16x3 = fp32 operands split into f16 hi/lo pairs, three f16 MFMA products per MAC, fp32 accumulation:
    same accuracy against fp64 as the all-fp32 kernel, ~2.9x its speed.  The front-ends
    re-run a batch in f32 automatically if an activation leaves f16's range (never seen on real networks)."""
    if _forced_precision is not None:
        return _forced_precision
    name = os.environ.get("INERF_PRECISION", "f16x3").lower()
    if name not in ("f32", "f16x3"):
        raise ValueError(f"INERF_PRECISION={name!r}: expected 'f32' or 'f16x3'")
    return PREC_F16X3 if name == "f16x3" else PREC_F32


def net_desc(variant, n_classes=0, l_xyz=10, l_dir=4, xyz_div=1.0, precision=None):
    prec = default_precision() if precision is None else int(precision)
    return NetDesc(int(variant), int(n_classes), int(l_xyz), int(l_dir), float(xyz_div), prec)
