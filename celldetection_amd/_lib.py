"""ctypes binding of libcpn_hip.so (the C ABI declared in include/cpn_hip.h).

The product path has NO CPU fallback: if the HIP library is missing or does not export the expected symbols,
importing the binding raises, and every op raises ``RuntimeError`` on failure with ``cpn_last_error()``.
"""
import ctypes
import os
from ctypes import (POINTER, Structure, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_void_p)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CPN_HIP_LIB') or os.path.join(HERE, 'libcpn_hip.so')  # env: kernel A/B tuning only

ABI_VERSION = 22
PRECISION_BF16, PRECISION_F32, PRECISION_FP8 = 0, 1, 2
E_INVALID, E_UNSUPPORTED, E_WORKSPACE, E_INTERNAL = -1, -2, -3, -4

OP_INPUT, OP_CONV, OP_MAXPOOL, OP_BILINEAR, OP_CONV_DEFERRED, OP_INPUT_STEM, OP_STEM7, OP_CONV_PAIR, OP_CONV_BRIDGE, OP_ACT = \
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH_SCALED = 0, 1, 2, 3
ACT_LEAKY_RELU, ACT_SILU, ACT_GELU, ACT_ELU, ACT_TANH, ACT_HARDSWISH, ACT_MISH, ACT_SELU, ACT_SOFTPLUS = 4, 5, 6, 7, 8, 9, 10, 11, 12
SUBPIXEL_NONE, SUBPIXEL_HEAD, SUBPIXEL_PHASE, SUBPIXEL_LATERAL, SUBPIXEL_SCATTER = 0, 1, 2, 3, 4
SUBPIXEL_BL_HEAD, SUBPIXEL_BL_PHASE, SUBPIXEL_BL_FRAME = 5, 6, 7
OUT_SCORES, OUT_LOCATIONS, OUT_FOURIER, OUT_REFINEMENT, OUT_UNCERTAINTY = 0, 1, 2, 3, 4
NUM_OUTPUTS = 5
# conv kernel modes (CPN_CONV_MODE_* of include/cpn_hip.h) as cpn_conv2d_kernel_info reports them
CONV_MODE_NAMES = {0: 'PW', 1: 'S1', 2: 'S2', 3: 'BL', 6: 'N', 7: 'S1F', 8: 'BR', 10: 'S1Q'}
# region properties (CPN_PROP_* of include/cpn_hip.h), in code order, and the intensity dtypes (CPN_PROPS_*)
PROP_NAMES = ('label', 'bbox', 'num_pixels', 'area', 'area_bbox', 'extent', 'equivalent_diameter_area', 'centroid',
              'centroid_local', 'inertia_tensor', 'inertia_tensor_eigvals', 'axis_major_length', 'axis_minor_length',
              'eccentricity', 'orientation', 'intensity_mean', 'intensity_min', 'intensity_max')
PROP_CODES = {name: code for code, name in enumerate(PROP_NAMES)}
PROPS_U8, PROPS_I16, PROPS_I32 = 0, 1, 2
# shape properties (CPN_SHAPE_* of include/cpn_hip.h), in code order
SHAPE_NAMES = ('label', 'num_pixels', 'perimeter', 'perimeter_crofton', 'euler_number', 'area_convex', 'solidity')
SHAPE_CODES = {name: code for code, name in enumerate(SHAPE_NAMES)}
# training objective (CPN_OBJECTIVE_* of include/cpn_hip.h)
OBJECTIVE_MAX_ITERATIONS, OBJECTIVE_META_WORDS = 64, 2
OBJECTIVE_FLAG_LABEL_RANGE, OBJECTIVE_FLAG_LABEL_ROWS, OBJECTIVE_FLAG_CLASS_RANGE = 1, 2, 4
# component labelling (CPN_COMPONENTS_* of include/cpn_hip.h)
COMPONENTS_EQUAL, COMPONENTS_NONZERO = 0, 1
COMPONENTS_MODES = {'equal': COMPONENTS_EQUAL, 'nonzero': COMPONENTS_NONZERO}
# trainable convolution (CPN_CONV_PACK_* and the dtype codes of include/cpn_hip.h)
CONV_PACK_FORWARD, CONV_PACK_DGRAD = 0, 1
CONV_PACK_MODES = {'forward': CONV_PACK_FORWARD, 'dgrad': CONV_PACK_DGRAD}
CONV_TRAIN_F32, CONV_TRAIN_BF16 = 0, 1
# optimizer step (CPN_OPTIM_* of include/cpn_hip.h)
OPTIM_CHUNK, OPTIM_FLAG_SCALAR, OPTIM_TENSOR_BYTES = 8192, 1, 80


class TensorDesc(Structure):
    _fields_ = [('channels', c_int32), ('down', c_int32), ('scale', c_float)]


class OpDesc(Structure):
    _fields_ = [('op', c_int32), ('src0', c_int32), ('src1', c_int32), ('res', c_int32), ('dst', c_int32),
                ('up0', c_int32), ('up1', c_int32), ('res_up', c_int32), ('c0_used', c_int32),
                ('kh', c_int32), ('kw', c_int32), ('stride', c_int32), ('pad', c_int32),
                ('bundles', c_int32), ('cin_b', c_int32), ('cout_b', c_int32),
                ('weight_offset', c_int64), ('bias_offset', c_int64),
                ('act', c_int32), ('act_scale', c_float), ('out_index', c_int32), ('cout_real', c_int32),
                ('dst_coff', c_int32), ('in_channels', c_int32),
                ('fuse_weight_offset', c_int64), ('fuse_bias_offset', c_int64), ('fuse_cout', c_int32),
                ('fuse_act', c_int32), ('fuse_act_scale', c_float), ('mult_offset', c_int32), ('subpixel', c_int32), ('alt', c_int32)]


class ObjectiveArgs(Structure):
    """CpnObjectiveArgs of include/cpn_hip.h (section "Training objective")."""
    _fields_ = [(n, c_void_p) for n in ('scores', 'locations', 'refinement', 'fourier', 'labels', 't_fourier', 't_locations',
                                        't_contours', 't_classes', 'cos_table', 'sin_table', 'bucket_index', 'bucket_weight',
                                        'order_weights', 'g_scores', 'g_locations', 'g_refinement', 'g_fourier',
                                        'detail_proposals', 'detail_refined', 'detail_boxes')] + \
               [(n, c_double) for n in ('w_fourier', 'w_location', 'w_contour', 'w_score_fg', 'w_score_bg', 'w_refinement',
                                        'w_iou')] + \
               [(n, c_int32) for n in ('N', 'score_channels', 'h', 'w', 'H', 'W', 'order_total', 'order', 'samples', 'K',
                                       'iterations', 'buckets', 'labels_i64', 'reserved')]


# every symbol include/cpn_hip.h declares: (name, restype, argtypes)
_SIGNATURES = [
    ('cpn_last_error', c_char_p, []),
    ('cpn_abi_version', ctypes.c_int, []),
    ('cpn_plan_create', ctypes.c_int, [POINTER(c_void_p), POINTER(TensorDesc), c_int32, POINTER(OpDesc), c_int32,
                                       c_void_p, c_size_t, c_void_p, c_size_t, c_int32]),
    ('cpn_plan_destroy', None, [c_void_p]),
    ('cpn_plan_workspace_bytes', c_int64, [c_void_p, c_int32, c_int32, c_int32]),
    ('cpn_plan_output_dims', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32)]),
    ('cpn_plan_max_tensor_elements', c_int64, [c_void_p, c_int32, c_int32]),
    ('cpn_plan_executed_flops', c_double, [c_void_p, c_int32, c_int32, c_int32]),
    ('cpn_plan_run', ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64,
                                    POINTER(c_void_p), c_void_p, c_void_p]),
    ('cpn_plan_run_stats', ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64,
                                          POINTER(c_void_p), c_void_p, c_void_p, c_void_p]),
    ('cpn_plan_num_ops', ctypes.c_int, [c_void_p]),
    ('cpn_plan_run_timed', ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64,
                                          POINTER(c_void_p), c_void_p, c_void_p, POINTER(c_float), POINTER(c_double)]),
    ('cpn_conv2d', ctypes.c_int, [POINTER(OpDesc), c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p,
                                  c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    ('cpn_conv2d_fp8', ctypes.c_int, [POINTER(OpDesc), c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p,
                                      c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_float, c_float,
                                      c_void_p]),
    ('cpn_conv2d_kernel_info', ctypes.c_int, [POINTER(OpDesc), c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                              c_int32, POINTER(c_int32)]),
    ('cpn_convert_input_stem', ctypes.c_int, [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                              c_void_p]),
    ('cpn_stem7', ctypes.c_int, [POINTER(OpDesc), c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                 c_float, c_void_p]),
    ('cpn_conv_pair', ctypes.c_int, [POINTER(OpDesc), c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                     c_void_p, c_void_p, c_void_p]),
    ('cpn_conv_bridge', ctypes.c_int, [POINTER(OpDesc), c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_int32,
                                       c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    ('cpn_maxpool2d', ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                     c_int32, c_void_p]),
    ('cpn_resize_bilinear', ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                           c_void_p]),
    ('cpn_convert_input', ctypes.c_int, [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                         c_void_p, c_void_p]),
    ('cpn_compact_workspace_bytes', c_int64, [c_int32, c_int32, c_int32]),
    ('cpn_compact', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_float, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
    ('cpn_decode', ctypes.c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                  c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_int32, c_void_p, c_void_p, c_void_p]),
    ('cpn_decode_gathered', ctypes.c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                           c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_int32, c_void_p, c_void_p, c_void_p]),
    ('cpn_sparse_heads', ctypes.c_int, [POINTER(OpDesc), POINTER(OpDesc), c_void_p, c_int32, c_int32, c_int32, c_int32,
                                        c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ('cpn_plan_tensor_info', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, POINTER(c_int64),
                                            POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    ('cpn_fouriers2contours', ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                             c_void_p, c_void_p]),
    ('cpn_local_refinement', ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32,
                                            c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    ('cpn_class_scores', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p]),
    ('cpn_certainty_mask', ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p,
                                          c_void_p]),
    ('cpn_gather_channels', ctypes.c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p,
                                           c_void_p]),
    ('cpn_nms_workspace_bytes', c_int64, [c_int64, c_int64, c_int32]),
    ('cpn_nms', ctypes.c_int, [c_void_p, c_void_p, c_int64, POINTER(c_int64), c_void_p, c_int32, c_float, c_void_p,
                               c_void_p, c_void_p, c_int64, c_void_p]),
    ('cpn_box_votes', ctypes.c_int, [c_void_p, c_int64, c_float, c_void_p, c_void_p]),
    ('cpn_border_keep', ctypes.c_int, [c_void_p, c_int64, c_int32, c_float, c_float, c_float, c_float, c_float,
                                       c_int32, c_void_p, c_void_p]),
    ('cpn_resize_bilinear_f32', ctypes.c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32,
                                               c_void_p]),
    ('cpn_resize_f32', ctypes.c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    ('cpn_border_keep_batched', ctypes.c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_int32,
                                               c_float, c_float, c_float, c_void_p, c_void_p]),
    ('cpn_histogram', ctypes.c_int, [c_void_p, c_int32, c_int64, c_void_p, c_void_p]),
    ('cpn_rescale_to_uint8', ctypes.c_int, [c_void_p, c_int32, c_int64, c_double, c_double, c_void_p, c_void_p]),
    ('cpn_debug_clock_probe', ctypes.c_int, [POINTER(ctypes.c_uint64), c_int32]),
    ('cpn_window_any', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p]),
    ('cpn_labels_prepare', ctypes.c_int, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                          c_void_p, c_void_p]),
    ('cpn_labels_bin', ctypes.c_int, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    ('cpn_labels_cell_bounds', ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    ('cpn_labels_round', ctypes.c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32,
                                        c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int32), c_int32, c_double,
                                        c_void_p]),
    ('cpn_nms_binned_workspace_bytes', c_int64, [c_int64, c_int64]),
    ('cpn_nms_binned', ctypes.c_int, [c_void_p, c_void_p, c_int64, c_float, c_int64, c_void_p, c_void_p,
                                      POINTER(c_int64), POINTER(c_int64), POINTER(c_int32), c_void_p, c_int64,
                                      c_void_p]),
    ('cpn_eval_workspace_bytes', c_int64, [c_int64, c_int64, c_int64]),
    ('cpn_eval_pairs', ctypes.c_int, [c_void_p, c_int32, c_void_p, c_int32, c_int64, c_int64, c_void_p, c_int64, c_void_p]),
    ('cpn_eval_table_status', ctypes.c_int, [c_void_p, c_int64, POINTER(c_int64), c_void_p]),
    ('cpn_eval_compact', ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    ('cpn_eval_unions', ctypes.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ('cpn_eval_select', ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_double, c_void_p,
                                       c_void_p, c_int64, POINTER(c_int64), c_void_p]),
    ('cpn_flat_workspace_bytes', c_int64, [c_int32, c_int32]),
    ('cpn_flat_classify', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int64,
                                         POINTER(c_int64), c_void_p]),
    ('cpn_flat_step', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64,
                                     POINTER(c_int64), c_void_p]),
    ('cpn_flat_finish', ctypes.c_int, [c_void_p, c_int32, c_int32, c_void_p, c_int64, c_void_p]),
    ('cpn_props_workspace_bytes', c_int64, [c_int64, c_int32]),
    ('cpn_props_columns', c_int32, [POINTER(c_int32), c_int32, c_int32]),
    ('cpn_props_accumulate', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_int64, c_void_p,
                                            c_int64, c_void_p]),
    ('cpn_props_table_status', ctypes.c_int, [c_void_p, c_int64, POINTER(c_int64), c_void_p]),
    ('cpn_props_compact_sort', ctypes.c_int, [c_void_p, c_int64, c_int32, c_int64, c_void_p]),
    ('cpn_props_finalise', ctypes.c_int, [c_void_p, c_int64, c_int32, c_int64, POINTER(c_int32), c_int32, c_double, c_double,
                                          c_void_p, c_int64, c_void_p]),
    ('cpn_shape_workspace_bytes', c_int64, [c_int64]),
    ('cpn_shape_columns', c_int32, [POINTER(c_int32), c_int32]),
    ('cpn_shape_heights', ctypes.c_int, [c_void_p, c_int64, c_int32, c_int64, c_void_p, c_void_p]),
    ('cpn_shape_accumulate', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int64, c_int32, c_int64, c_void_p,
                                            c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    ('cpn_shape_hull_scratch_bytes', c_int64, [c_int64, c_int64]),
    ('cpn_shape_hull', ctypes.c_int, [c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    ('cpn_shape_finalise', ctypes.c_int, [c_void_p, c_int64, c_int32, c_int64, c_void_p, c_void_p, POINTER(c_int32), c_int32,
                                          c_double, c_double, c_void_p, c_int64, c_void_p]),
    ('cpn_overlay_bin_count', ctypes.c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    ('cpn_overlay_bin_fill', ctypes.c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int64,
                                            c_void_p]),
    ('cpn_overlay_paint', ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                         c_void_p, c_void_p, POINTER(ctypes.c_uint32), c_void_p]),
    ('cpn_label_cmap', ctypes.c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p,
                                      POINTER(c_int32), c_void_p]),
    ('cpn_contours_workspace_bytes', c_int64, [c_int64]),
    ('cpn_contours_components', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int64, POINTER(c_int64),
                                               c_void_p]),
    ('cpn_contours_table', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                          c_int64, POINTER(c_int64), c_void_p]),
    ('cpn_contours_count', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_int64, POINTER(c_int64), c_void_p]),
    ('cpn_contours_write', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_int64, c_void_p]),
    ('cpn_resample_contours', ctypes.c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_double, c_void_p, c_void_p,
                                             c_void_p]),
    ('cpn_efd_workspace_bytes', c_int64, [c_int64, c_int64, c_int32]),
    ('cpn_efd', ctypes.c_int, [c_void_p, c_int32, c_void_p, c_int64, c_int64, c_int32, c_double, c_int32, c_void_p, c_int64, c_void_p,
                               c_void_p, POINTER(c_int64), c_void_p]),
    ('cpn_label_distances_workspace_bytes', c_int64, [c_int32, c_int32]),
    ('cpn_label_distances_table_bytes', c_int64, [c_int64]),
    ('cpn_label_distances_classify', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64,
                                                    POINTER(c_int64), c_void_p]),
    ('cpn_label_distances_step', ctypes.c_int, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64,
                                                POINTER(c_int64), c_void_p]),
    ('cpn_label_distances_reduce', ctypes.c_int, [c_int32, c_int32, c_void_p, c_int64, c_void_p, c_int64, POINTER(c_int64),
                                                  c_void_p]),
    ('cpn_label_distances_finalise', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64,
                                                    c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    ('cpn_label_distances_mask', ctypes.c_int, [c_void_p, c_int32, c_int64, c_void_p, c_float, c_float, c_void_p, c_void_p]),
    ('cpn_label_remap', ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_void_p]),
    ('cpn_objective_head_workspace_bytes', c_int64, [c_int32, c_int32, c_int32]),
    ('cpn_objective_head', ctypes.c_int, [POINTER(ObjectiveArgs), c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    ('cpn_objective_workspace_bytes', c_int64, [POINTER(ObjectiveArgs), c_int64]),
    ('cpn_objective_proposals', ctypes.c_int, [POINTER(ObjectiveArgs), c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p,
                                               c_int64, c_void_p, c_void_p]),
    ('cpn_components_workspace_bytes', c_int64, [c_int32, c_int32, c_int32]),
    ('cpn_components_label', ctypes.c_int, [c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                            c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    ('cpn_conv_train_pack', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    ('cpn_conv_wgrad_workspace_bytes', c_int64, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    ('cpn_conv_wgrad', ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                      c_int32, c_void_p, c_int32, c_void_p, c_int64, c_void_p]),
    ('cpn_conv_wgrad_info', ctypes.c_int, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32)]),
    ('cpn_bn_info', ctypes.c_int, [c_int64, c_int64, c_int64, POINTER(c_int64)]),
    ('cpn_bn_workspace_bytes', c_int64, [c_int64, c_int64, c_int64]),
    ('cpn_bn_train_stats', ctypes.c_int, [c_void_p, c_int32, c_int64, c_int64, c_int64, c_void_p, c_int32, c_void_p, c_int32, c_void_p,
                                          c_void_p, c_int32, c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_int64, c_void_p]),
    ('cpn_bn_eval_coeffs', ctypes.c_int, [c_int64, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_double,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ('cpn_bn_apply', ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int32, c_void_p]),
    ('cpn_bn_backward_reduce', ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int32,
                                              c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p,
                                              c_void_p, c_int64, c_void_p]),
    ('cpn_bn_backward_input', ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                             c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ('cpn_tail_info', ctypes.c_int, [c_int64, c_int64, c_int32, c_int32, c_int64, POINTER(c_int64)]),
    ('cpn_tail_workspace_bytes', c_int64, [c_int64, c_int64, c_int32, c_int32, c_int64]),
    ('cpn_tail_forward', ctypes.c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_float, c_int64, c_int64, c_int32,
                                        c_int32, c_void_p, c_int32, c_void_p]),
    ('cpn_tail_backward', ctypes.c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_float, c_int64, c_int64, c_int32,
                                         c_int32, c_int64, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int64,
                                         c_void_p]),
    ('cpn_grouped_conv_pack', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    ('cpn_grouped_conv_dilate', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    ('cpn_grouped_conv_wgrad_workspace_bytes', c_int64, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    ('cpn_grouped_conv_wgrad_info', ctypes.c_int, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32)]),
    ('cpn_grouped_conv_wgrad', ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                              c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int64, c_void_p]),
    ('cpn_residual_bn_apply', ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                             c_int32, c_void_p]),
    ('cpn_residual_bn_backward_reduce', ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int64, c_int64,
                                                       c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
                                                       c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_void_p]),
    ('cpn_subsample2d', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    ('cpn_conv2d_sized', ctypes.c_int, [POINTER(OpDesc), c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p,
                                        c_int32, c_int32, c_int32, c_int32, POINTER(c_int32), c_void_p, c_void_p, c_void_p]),
    ('cpn_cat_conv_wgrad_workspace_bytes', c_int64, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                                     c_int32]),
    ('cpn_cat_conv_wgrad_info', ctypes.c_int, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                               c_int32, POINTER(c_int32)]),
    ('cpn_cat_conv_wgrad', ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                          c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int64,
                                          c_void_p]),
    ('cpn_nearest_sum', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p]),
    ('cpn_resized_conv_wgrad_workspace_bytes', c_int64, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                                         c_int32]),
    ('cpn_resized_conv_wgrad_info', ctypes.c_int, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                                   POINTER(c_int32)]),
    ('cpn_resized_conv_wgrad', ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                              c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int64, c_void_p]),
    ('cpn_bilinear_sum', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p]),
    ('cpn_bilinear_sum_f32', ctypes.c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p]),
    ('cpn_stem_train_pack', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    ('cpn_stem_train_forward', ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    ('cpn_stem_wgrad_info', ctypes.c_int, [c_int32, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32)]),
    ('cpn_stem_wgrad_workspace_bytes', c_int64, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    ('cpn_stem_wgrad', ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32,
                                      c_void_p, c_int32, c_void_p, c_int64, c_void_p]),
    ('cpn_maxpool2d_indexed', ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                             c_void_p, c_void_p]),
    ('cpn_maxpool2d_backward', ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                              c_int32, c_void_p, c_void_p]),
    ('cpn_optim_info', ctypes.c_int, [POINTER(c_int64), c_int32, POINTER(c_int64), POINTER(c_int64)]),
    ('cpn_optim_chunk_map', ctypes.c_int, [POINTER(c_int64), c_int32, c_void_p, c_int64]),
    ('cpn_optim_upload', ctypes.c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    ('cpn_optim_sumsq', ctypes.c_int, [c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_void_p]),
    ('cpn_optim_norm', ctypes.c_int, [c_void_p, c_int64, c_double, c_void_p, c_void_p]),
    ('cpn_optim_adamw', ctypes.c_int, [c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_int32, c_void_p]),
    ('cpn_optim_scale', ctypes.c_int, [c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_void_p]),
]

EXPORTED_SYMBOLS = tuple(s[0] for s in _SIGNATURES)

_lib = None


def load():
    """Loads libcpn_hip.so; raises RuntimeError (never falls back) when it is missing or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise RuntimeError(f'{LIB_PATH} not found: build the HIP extension first '
                           f'(python -m celldetection_amd.build); there is no CPU fallback.')
    lib = ctypes.CDLL(LIB_PATH)
    for name, restype, argtypes in _SIGNATURES:
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError(f'{LIB_PATH} does not export {name}; rebuild it.') from e
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.cpn_abi_version() != ABI_VERSION:
        raise RuntimeError(f'libcpn_hip.so ABI version {lib.cpn_abi_version()} != expected {ABI_VERSION}; rebuild it.')
    _lib = lib
    return lib


def check(rc, what=''):
    if rc != 0:
        msg = load().cpn_last_error()
        raise RuntimeError(f'libcpn_hip {what} failed (code {rc}): {msg.decode() if msg else "?"}')


def stream_ptr():
    import torch
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device/host pointer of a tensor (None -> NULL)."""
    return c_void_p(0 if t is None else t.data_ptr())


def conv_kernel_info(op, precision, n, hin, win, c0_stride, c1_stride=0, res_stride=0, dst_stride=0):
    """The kernel cpn_conv2d (PRECISION_BF16; a CONV_BRIDGE descriptor: cpn_conv_bridge) or cpn_conv2d_fp8 (PRECISION_FP8)
    would launch for this descriptor, these channel strides and this input size -> (mode name, TH, BN, WM, WN): the
    instantiation conv_igemm_kernel<TH, BN, WM, WN, mode>.  Host arithmetic only: needs no GPU.  Raises like the launch
    itself for a call it rejects."""
    info = (c_int32 * 5)()
    check(load().cpn_conv2d_kernel_info(op, precision, c0_stride, c1_stride, res_stride, dst_stride, n, hin, win, info),
          'conv2d_kernel_info')
    return (CONV_MODE_NAMES[info[0]],) + tuple(info[1:])
