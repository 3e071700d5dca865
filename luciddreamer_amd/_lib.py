"""ctypes binding of liblucid_raster.so (the C-ABI declared in include/lucid_raster.h).

This is the reference-side binding a maintainer would add in place of the pybind11 module
`depth_diff_gaussian_rasterization_min._C` (RAST/ext.cpp:15-19).  There is NO CPU fallback: if the
HIP library is missing this module raises, and tensors that are not on a HIP device are rejected.
"""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# one library instance per process: the compiled binding (_C_ext) is linked against this very file ($ORIGIN/lib).
# LR_LIB_DIR (with LD_LIBRARY_PATH pointing at the same directory, so that _C_ext resolves to the same file) switches the
# process to another build of it -- the diagnostics build of tools/ab_bench.py (tools/diag_env.sh sets both).
LIB_PATH = os.path.join(os.environ.get("LR_LIB_DIR") or os.path.join(_HERE, "lib"), "liblucid_raster.so")

ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)

LR_ERR_INVALID_ARG = -10
LR_ERR_HIP = -11
LR_ERR_PREFILTERED = -12
LR_ERR_OVERFLOW = -13
LR_ERR_ALLOC = -14
LR_NUM_RENDERED_ON_DEVICE = -1

_lib = None
_lock = threading.Lock()

EXPORTS = ("lr_last_error", "lr_version", "lr_geom_bytes", "lr_img_bytes", "lr_binning_bytes", "lr_forward",
           "lr_backward", "lr_view_forward", "lr_view_backward", "lr_render_alpha", "lr_render_median", "lr_median_backward",
           "lr_render_distortion", "lr_distortion_backward", "lr_render_normals", "lr_render_normals_backward",
           "lr_render_geometry", "lr_geometry_backward",
           "lr_features_workspace_bytes", "lr_render_features", "lr_render_features_backward",
           "lr_mark_visible", "lr_check",
           "lr_dist2_workspace_bytes", "lr_dist2",
           "lr_dist2_workspace_layout",
           "lr_profile_enable", "lr_profile_stage_name", "lr_profile_read", "lr_tune_set", "lr_last_launch_shapes", "lr_last_forward_channels",
           "lr_request_early_header",
           "lr_take_early_ticket", "lr_forward_ticket", "lr_backward_wait_event", "lr_step_begin", "lr_step_end", "lr_step_abort",
           "lr_views_workspace_bytes", "lr_views_accumulate", "lr_views_check",
           "lr_loss_workspace_bytes", "lr_l1_dssim_forward", "lr_l1_dssim_backward", "lr_l1_dssim_backward_weights",
           "lr_select_workspace_bytes", "lr_select_rows", "lr_pack_ply_rows", "lr_adam_step", "lr_adam_step_masked", "lr_densify_stats",
           "lr_depth_l1_workspace_bytes", "lr_depth_l1_forward", "lr_depth_l1_backward",
           "lr_depth_pearson_workspace_bytes", "lr_depth_pearson_forward", "lr_depth_pearson_backward",
           "lr_video_workspace_bytes", "lr_frames_to_u8", "lr_depth_colorize",
           "lr_masked_l1_dssim_forward", "lr_masked_l1_dssim_backward", "lr_alpha_hole_workspace_bytes", "lr_alpha_hole_forward",
           "lr_alpha_hole_backward", "lr_set_antialiasing", "lr_get_antialiasing",
           "lr_mcmc_workspace_bytes", "lr_mcmc_relocate", "lr_mcmc_noise", "lr_mcmc_reg_grad",
           "lr_filter3d_workspace_bytes", "lr_filter3d_update", "lr_filter3d_apply_forward", "lr_filter3d_apply_backward",
           "lr_reproject_workspace_bytes", "lr_reproject", "lr_lift",
           "lr_dream_workspace_bytes", "lr_dream_scale_sums", "lr_dream_correspond", "lr_dream_lift", "lr_scatter_interpolate",
           "lr_normals_workspace_bytes", "lr_depth_normals", "lr_depth_normals_backward", "lr_normal_loss_forward",
           "lr_normal_loss_backward",
           "lr_smooth_workspace_bytes", "lr_smooth_forward", "lr_smooth_backward",
           "lr_tsdf_workspace_bytes", "lr_tsdf_integrate", "lr_tsdf_extract_count", "lr_tsdf_extract_emit",
           "lr_mesh_workspace_bytes", "lr_mesh_components", "lr_mesh_filter_count", "lr_mesh_filter_emit", "lr_mesh_vertex_normals")

# lr_views_workspace_bytes / lr_views_check `parts`: what a step's workspace slots hold besides a view's scratch
LR_VIEWS_LOSS, LR_VIEWS_DEPTH_LOSS, LR_VIEWS_MASK_LOSS = 1, 2, 4
LR_VIEWS_DEPTH_PEARSON = 16         # the slot's depth-loss workspace is the Pearson term's (8 is not a flag)
LR_VIEWS_GEOM = 64                  # the slot holds the geometry pass's maps, upstream images and workspace (32 is not a flag)
# lr_views_args.depth_loss: the depth term of the fused training step
LR_DEPTH_LOSS_L1, LR_DEPTH_LOSS_PEARSON = 0, 1


class ViewsArgs(ctypes.Structure):
    """lr_views_args of include/lucid_raster.h, field for field (tests/test_views_args_cpu.py compares the offsets with the
    host compiler's).  `[]` marks HOST arrays of n_views entries."""
    _vp, _ci, _cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    _fields_ = [("struct_bytes", ctypes.c_size_t),
                # the views
                ("n_views", _ci), ("viewmatrices", _vp), ("projmatrices", _vp), ("cam_positions", _vp),      # [] [] []
                ("tan_fovx", _vp), ("tan_fovy", _vp),                                                       # float[] float[]
                # the scene
                ("P", _ci), ("D", _ci), ("M", _ci), ("background", _vp), ("width", _ci), ("height", _ci),
                ("means3D", _vp), ("shs", _vp), ("colors_precomp", _vp), ("opacities", _vp), ("scales", _vp),
                ("rotations", _vp), ("cov3D_precomp", _vp), ("scale_modifier", _cf),
                # fixed upstream gradients
                ("dL_dpix", _vp), ("dL_ddepth", _vp), ("dL_dalpha", _vp),                                    # [] [] []
                # the fused training step
                ("targets", _vp), ("lambda_dssim", _cf), ("depth_targets", _vp), ("depth_weight", _cf),      # [] . [] .
                ("masks", _vp), ("alpha_weight", _cf), ("out_losses", _vp),                                  # [] . device
                # optional per-view outputs
                ("out_color", _vp), ("out_depth", _vp), ("out_alpha", _vp), ("out_radii", _vp),              # [] [] [] []
                # the accumulators
                ("acc_mean2D", _vp), ("acc_opacity", _vp), ("acc_color", _vp), ("acc_mean3D", _vp),
                ("acc_cov3D", _vp), ("acc_sh", _vp), ("acc_scale", _vp), ("acc_rot", _vp),
                # densification statistics [P]: all three or none; stat_absgrad selects the absolute gradient's norm
                ("stat_grad_accum", _vp), ("stat_denom", _vp), ("stat_max_radii", _vp), ("stat_absgrad", _ci),
                ("workspace", _vp), ("workspace_bytes", ctypes.c_size_t), ("binning_capacity", ctypes.c_longlong),
                ("n_streams", _ci), ("stream", _vp),
                # LR_DEPTH_LOSS_*; the last member, so that sizeof grew with it (see the header)
                ("depth_loss", _ci)]

    def __init__(self, **fields):
        super().__init__(struct_bytes=ctypes.sizeof(type(self)), **fields)


class ViewsGeomArgs(ViewsArgs):
    """lr_views_geom_args: lr_views_args as its first member (`base`; here the base class, so its members read as this struct's
    own) and the two geometry regularisers' members behind it.  struct_bytes is this struct's size; lr_views_accumulate takes it
    where it takes a ViewsArgs.  All zero / NULL: the step without the terms."""
    _vp, _cf = ctypes.c_void_p, ctypes.c_float
    _fields_ = [("distortion_weight", _cf), ("distortion_map", _cf * 3), ("normal_consistency_weight", _cf),
                ("out_distortion", _vp), ("out_normals", _vp)]                                             # [] []


class View(ctypes.Structure):
    """lr_view: the scene and camera of one view (raw != 0: the stored GaussianModel tensors; see the header)."""
    _vp, _ci, _cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    _fields_ = [("P", _ci), ("D", _ci), ("M", _ci), ("raw", _ci),
                ("background", _vp), ("width", _ci), ("height", _ci),
                ("means3D", _vp), ("shs", _vp), ("sh_rest", _vp), ("colors_precomp", _vp), ("opacities", _vp), ("scales", _vp),
                ("scale_modifier", _cf), ("rotations", _vp), ("cov3D_precomp", _vp),
                ("viewmatrix", _vp), ("projmatrix", _vp), ("campos", _vp), ("tan_fovx", _cf), ("tan_fovy", _cf)]


class ForwardArgs(ctypes.Structure):
    """lr_forward_args, field for field (tests/test_view_args_cpu.py compares the offsets with the host compiler's)."""
    _vp, _ci = ctypes.c_void_p, ctypes.c_int
    _fields_ = [("struct_bytes", ctypes.c_size_t), ("view", View),
                ("geom_alloc", ALLOC_FN), ("geom_user", _vp), ("binning_alloc", ALLOC_FN), ("binning_user", _vp),
                ("img_alloc", ALLOC_FN), ("img_user", _vp), ("prefiltered", _ci),
                ("out_color", _vp), ("out_depth", _vp), ("radii", _vp),
                ("debug", _ci), ("binning_capacity", ctypes.c_longlong), ("stream", _vp)]

    def __init__(self, **fields):
        super().__init__(struct_bytes=ctypes.sizeof(ForwardArgs), **fields)


class BackwardArgs(ctypes.Structure):
    """lr_backward_args, field for field.  Which optional pointers are given selects the depth / alpha / absgrad mode."""
    _vp, _ci = ctypes.c_void_p, ctypes.c_int
    _fields_ = [("struct_bytes", ctypes.c_size_t), ("view", View),
                ("R", _ci), ("radii", _vp), ("geom_buffer", _vp), ("binning_buffer", _vp), ("image_buffer", _vp),
                ("dL_dpix", _vp), ("dL_depths", _vp), ("depth_image", _vp), ("dL_dalpha", _vp),
                ("dL_dmean2D", _vp), ("dL_dmean2D_abs", _vp), ("dL_dconic", _vp), ("dL_dopacity", _vp), ("dL_dcolor", _vp),
                ("dL_dmean3D", _vp), ("dL_dcov3D", _vp), ("dL_dsh", _vp), ("dL_dsh_rest", _vp), ("dL_dscale", _vp),
                ("dL_drot", _vp),
                ("debug", _ci), ("binning_capacity", ctypes.c_longlong), ("accumulate_mask", ctypes.c_uint), ("stream", _vp)]

    def __init__(self, **fields):
        super().__init__(struct_bytes=ctypes.sizeof(BackwardArgs), **fields)


# The passes behind a finished forward (include/lucid_raster.h): their argument structs are built from two runs of members every
# one of them repeats.  tests/test_{median,distort,render_normals,features,geom_views}_cpu.py compare each struct's offsets with
# the host compiler's.
_vp, _ci, _cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
_BUFFERS = [("geom_buffer", _vp), ("binning_buffer", _vp), ("image_buffer", _vp)]
_CAPACITY = [("binning_capacity", ctypes.c_longlong)]
# the state a forward left: its three buffers and the capacity it ran under -- with P, width, height between them where the struct
# has no lr_view of its own
FORWARD_STATE = _BUFFERS + _CAPACITY
FORWARD_STATE_PWH = _BUFFERS + [("P", _ci), ("width", _ci), ("height", _ci)] + _CAPACITY
# the gradient outputs of a backward, as lr_backward_args names them, and the end of the struct
GRAD_OUTPUTS = [("dL_dmean2D", _vp), ("dL_dconic", _vp), ("dL_dopacity", _vp), ("dL_dcolor", _vp), ("dL_dmean3D", _vp),
                ("dL_dcov3D", _vp), ("dL_dsh", _vp), ("dL_dsh_rest", _vp), ("dL_dscale", _vp), ("dL_drot", _vp),
                ("accumulate_mask", ctypes.c_uint), ("stream", _vp)]
_MAP = [("map_c0", _cf), ("map_c1", _cf), ("map_c2", _cf)]


def _struct_bytes_first(cls):
    """Class decorator of the ten: struct_bytes, the first member of each, is filled in with the class's own size."""
    def __init__(self, **fields):
        ctypes.Structure.__init__(self, struct_bytes=ctypes.sizeof(cls), **fields)
    cls.__init__ = __init__
    return cls


_SIZE, _VIEW, _STREAM = [("struct_bytes", ctypes.c_size_t)], [("view", View)], [("stream", _vp)]


@_struct_bytes_first
class MedianArgs(ctypes.Structure):
    """lr_median_args, field for field."""
    _fields_ = _SIZE + FORWARD_STATE_PWH + [("out_median_depth", _vp), ("out_ids", _vp)] + _STREAM


@_struct_bytes_first
class MedianBackwardArgs(ctypes.Structure):
    """lr_median_backward_args, field for field."""
    _fields_ = (_SIZE + FORWARD_STATE_PWH +
                [("radii", _vp), ("ids", _vp), ("dL_dmedian", _vp), ("viewmatrix", _vp), ("dL_dmean3D", _vp), ("accumulate", _ci)] +
                _STREAM)


@_struct_bytes_first
class DistortionArgs(ctypes.Structure):
    """lr_distortion_args, field for field."""
    _fields_ = _SIZE + FORWARD_STATE_PWH + _MAP + [("out_distortion", _vp), ("out_moments", _vp)] + _STREAM


@_struct_bytes_first
class DistortionBackwardArgs(ctypes.Structure):
    """lr_distortion_backward_args, field for field."""
    _fields_ = (_SIZE + _VIEW + FORWARD_STATE + [("dL_ddistortion", _vp), ("moments", _vp), ("distortion", _vp)] + _MAP +
                GRAD_OUTPUTS)


@_struct_bytes_first
class NormalsRenderArgs(ctypes.Structure):
    """lr_normals_render_args, field for field."""
    _fields_ = _SIZE + _VIEW + [("radii", _vp)] + FORWARD_STATE + [("out_normals", _vp), ("out_gauss_normals", _vp)] + _STREAM


_NORMALS_UPSTREAM = [("dL_dnormals", _vp), ("normals", _vp), ("gauss_normals", _vp), ("radii", _vp), ("dL_dgauss_normal", _vp)]


@_struct_bytes_first
class NormalsRenderBackwardArgs(ctypes.Structure):
    """lr_normals_render_backward_args, field for field."""
    _fields_ = _SIZE + _VIEW + FORWARD_STATE + _NORMALS_UPSTREAM + GRAD_OUTPUTS


LR_FEATURE_MAX_CHANNELS = 256       # include/lucid_raster.h
LR_ACC_FEATURES = 1 << 9            # accumulate_mask of lr_render_features_backward: dL_dfeatures is added to
LR_FEATURE_CHUNK = 16               # channels per tile walk (csrc/render_features.hip FTR_K): C channels cost ceil(C / 16) walks each way


@_struct_bytes_first
class FeatureRenderArgs(ctypes.Structure):
    """lr_feature_render_args, field for field."""
    _fields_ = (_SIZE + _VIEW + [("radii", _vp)] + FORWARD_STATE +
                [("features", _vp), ("channels", _ci), ("out_features", _vp)] + _STREAM)


@_struct_bytes_first
class FeatureRenderBackwardArgs(ctypes.Structure):
    """lr_feature_render_backward_args, field for field."""
    _fields_ = (_SIZE + _VIEW + FORWARD_STATE +
                [("features", _vp), ("channels", _ci), ("dL_dout_features", _vp), ("out_features", _vp), ("radii", _vp),
                 ("dL_dfeatures", _vp), ("workspace", _vp), ("workspace_bytes", ctypes.c_size_t)] + GRAD_OUTPUTS)


@_struct_bytes_first
class GeometryArgs(ctypes.Structure):
    """lr_geometry_args, field for field."""
    _fields_ = (_SIZE + _VIEW + [("radii", _vp)] + FORWARD_STATE + _MAP +
                [("out_distortion", _vp), ("out_moments", _vp), ("out_normals", _vp), ("out_gauss_normals", _vp)] + _STREAM)


@_struct_bytes_first
class GeometryBackwardArgs(ctypes.Structure):
    """lr_geometry_backward_args, field for field."""
    _fields_ = (_SIZE + _VIEW + FORWARD_STATE +
                [("dL_ddistortion", _vp), ("dL_ddistortion_scalar", _cf), ("moments", _vp), ("distortion", _vp)] + _MAP +
                _NORMALS_UPSTREAM + GRAD_OUTPUTS)


def distortion_map_coefficients(distortion_map):
    """(c0, c1, c2) of the mapped depth m = c0 + c1 z + c2 / z (include/lucid_raster.h) for "ndc" (2DGS's
    far / (far - near) (1 - near / z) with near = 0.2, far = 100), ("ndc", near, far), "linear" (m = z), or three numbers."""
    m = distortion_map
    if m == "linear":
        return 0.0, 1.0, 0.0
    if m == "ndc":
        m = ("ndc", 0.2, 100.0)
    if isinstance(m, (tuple, list)) and len(m) == 3 and m[0] == "ndc":
        near, far = float(m[1]), float(m[2])
        if not 0.0 < near < far:
            raise ValueError("distortion_map: need 0 < near < far")
        return far / (far - near), 0.0, -far * near / (far - near)
    if isinstance(m, (tuple, list)) and len(m) == 3 and all(isinstance(c, (int, float)) for c in m):
        return tuple(float(c) for c in m)
    raise ValueError('distortion_map must be "ndc", ("ndc", near, far), "linear" or three coefficients')


class McmcRelocateArgs(ctypes.Structure):
    """lr_mcmc_relocate_args, field for field (tests/test_mcmc_cpu.py compares the offsets with the host compiler's)."""
    _vp, _ci = ctypes.c_void_p, ctypes.c_int
    _fields_ = [("struct_bytes", ctypes.c_size_t), ("n", _ci), ("dst", _vp), ("src", _vp), ("P_rows", _ci), ("M", _ci),
                ("xyz", _vp), ("features_dc", _vp), ("features_rest", _vp), ("opacity", _vp), ("scaling", _vp), ("rotation", _vp),
                ("exp_avg", _vp * 6), ("exp_avg_sq", _vp * 6),
                ("min_opacity", ctypes.c_float), ("n_max", _ci),
                ("workspace", _vp), ("workspace_bytes", ctypes.c_size_t), ("stream", _vp)]

    def __init__(self, **fields):
        super().__init__(struct_bytes=ctypes.sizeof(McmcRelocateArgs), **fields)


class ReprojectArgs(ctypes.Structure):
    """lr_reproject_args, field for field (tests/test_reproject_cpu.py compares the offsets with the host compiler's).
    K, R, T are HOST float64 arrays; every out_* is optional."""
    _vp, _ci, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    _fields_ = [("struct_bytes", ctypes.c_size_t), ("n_points", _ll), ("points", _vp), ("point_stride", _ll),
                ("coord_stride", _ll), ("colors", _vp), ("n_frames", _ci), ("height", _ci), ("width", _ci),
                ("z_tolerance", ctypes.c_float), ("K", _vp), ("R", _vp), ("T", _vp),
                ("out_image", _vp), ("out_image_u8", _vp), ("out_mask", _vp), ("out_dilated", _vp), ("out_border", _vp),
                ("out_depth", _vp), ("out_valid", _vp), ("out_pix", _vp),
                ("workspace", _vp), ("workspace_bytes", ctypes.c_size_t), ("stream", _vp)]

    def __init__(self, **fields):
        super().__init__(struct_bytes=ctypes.sizeof(ReprojectArgs), **fields)


class DreamArgs(ctypes.Structure):
    """lr_dream_args, field for field (tests/test_dream_cpu.py compares the offsets with the host compiler's).  K, R, T, Kinv, Rinv
    and RinvT are HOST float64 arrays; each entry point reads its own members."""
    _vp, _ci, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    _fields_ = [("struct_bytes", ctypes.c_size_t), ("n_points", _ll), ("points", _vp), ("point_stride", _ll),
                ("coord_stride", _ll), ("valid", _vp), ("pix", _vp), ("height", _ci), ("width", _ci), ("depth", _vp),
                ("K", _vp), ("R", _vp), ("T", _vp), ("Kinv", _vp), ("Rinv", _vp), ("RinvT", _vp), ("scale", ctypes.c_double),
                ("corr", _vp), ("n_corr", _ll), ("out_su", _vp), ("out_sv", _vp), ("out_sval", _vp),
                ("out_sums", _vp), ("out_count", _vp), ("new_depth", _vp), ("out_points", _vp),
                ("workspace", _vp), ("workspace_bytes", ctypes.c_size_t), ("stream", _vp)]

    def __init__(self, **fields):
        super().__init__(struct_bytes=ctypes.sizeof(DreamArgs), **fields)


class ScatterArgs(ctypes.Structure):
    """lr_scatter_args, field for field."""
    _vp, _ci = ctypes.c_void_p, ctypes.c_int
    _fields_ = [("struct_bytes", ctypes.c_size_t), ("n_samples", ctypes.c_longlong), ("su", _vp), ("sv", _vp), ("sval", _vp),
                ("height", _ci), ("width", _ci), ("where", _vp), ("out", _vp), ("stream", _vp)]

    def __init__(self, **fields):
        super().__init__(struct_bytes=ctypes.sizeof(ScatterArgs), **fields)


class NormalsArgs(ctypes.Structure):
    """lr_normals_args, field for field (tests/test_normals_cpu.py compares the offsets with the host compiler's)."""
    _vp, _ci, _cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    _fields_ = [("struct_bytes", ctypes.c_size_t), ("height", _ci), ("width", _ci), ("tan_fovx", _cf), ("tan_fovy", _cf),
                ("depth", _vp), ("out_normals", _vp), ("dL_dnormals", _vp), ("target_normals", _vp), ("target_depth", _vp),
                ("pixel_weight", _vp), ("weight", _cf), ("upstream", _vp), ("out", _vp), ("dL_ddepth", _vp),
                ("dL_dtarget_depth", _vp), ("workspace", _vp), ("workspace_bytes", ctypes.c_size_t), ("stream", _vp)]

    def __init__(self, **fields):
        super().__init__(struct_bytes=ctypes.sizeof(NormalsArgs), **fields)


LR_SMOOTH_DIRECT, LR_SMOOTH_INVERSE = 0, 1          # lr_smooth_args.space


class SmoothArgs(ctypes.Structure):
    """lr_smooth_args, field for field (tests/test_smooth_cpu.py compares the offsets with the host compiler's)."""
    _vp, _ci, _cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    _fields_ = [("struct_bytes", ctypes.c_size_t), ("height", _ci), ("width", _ci), ("channels", _ci), ("guide_channels", _ci),
                ("map", _vp), ("guide", _vp), ("mask", _vp), ("order", _ci), ("space", _ci), ("positive_only", _ci),
                ("gamma", _cf), ("weight", _cf), ("upstream", _vp), ("out", _vp), ("dL_dmap", _vp),
                ("workspace", _vp), ("workspace_bytes", ctypes.c_size_t), ("stream", _vp)]

    def __init__(self, **fields):
        super().__init__(struct_bytes=ctypes.sizeof(SmoothArgs), **fields)


class TsdfVolumeDesc(ctypes.Structure):
    """lr_tsdf_volume, field for field: the lattice and its three device tensors."""
    _vp, _ci, _cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    _fields_ = [("origin", _cf * 3), ("voxel_size", _cf), ("nx", _ci), ("ny", _ci), ("nz", _ci), ("trunc", _cf),
                ("tsdf", _vp), ("weight", _vp), ("color", _vp)]


class TsdfIntegrateArgs(ctypes.Structure):
    """lr_tsdf_integrate_args, field for field (tests/test_tsdf_cpu.py compares the offsets with the host compiler's).
    K, R, T are HOST float64 arrays; color and pixel_weight are optional."""
    _vp, _ci, _cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    _fields_ = [("struct_bytes", ctypes.c_size_t), ("vol", TsdfVolumeDesc), ("n_frames", _ci), ("height", _ci), ("width", _ci),
                ("depth", _vp), ("color", _vp), ("pixel_weight", _vp), ("K", _vp), ("R", _vp), ("T", _vp),
                ("depth_max", _cf), ("max_weight", _cf), ("stream", _vp)]

    def __init__(self, **fields):
        super().__init__(struct_bytes=ctypes.sizeof(TsdfIntegrateArgs), **fields)


class TsdfExtractArgs(ctypes.Structure):
    """lr_tsdf_extract_args, field for field.  out_n_vertices / out_n_faces are HOST long long."""
    _vp, _ll = ctypes.c_void_p, ctypes.c_longlong
    _fields_ = [("struct_bytes", ctypes.c_size_t), ("vol", TsdfVolumeDesc), ("min_weight", ctypes.c_float),
                ("workspace", _vp), ("workspace_bytes", ctypes.c_size_t), ("out_n_vertices", _vp), ("out_n_faces", _vp),
                ("n_vertices", _ll), ("n_faces", _ll), ("out_vertices", _vp), ("out_colors", _vp), ("out_faces", _vp),
                ("stream", _vp)]

    def __init__(self, **fields):
        super().__init__(struct_bytes=ctypes.sizeof(TsdfExtractArgs), **fields)


class MeshComponentsArgs(ctypes.Structure):
    """lr_mesh_components_args, field for field (tests/test_mesh_cpu.py compares the offsets with the host compiler's)."""
    _vp, _ll = ctypes.c_void_p, ctypes.c_longlong
    _fields_ = [("struct_bytes", ctypes.c_size_t), ("n_vertices", _ll), ("n_faces", _ll), ("faces", _vp), ("vertex_labels", _vp),
                ("face_labels", _vp), ("component_faces", _vp), ("workspace", _vp), ("workspace_bytes", ctypes.c_size_t),
                ("stream", _vp)]

    def __init__(self, **fields):
        super().__init__(struct_bytes=ctypes.sizeof(MeshComponentsArgs), **fields)


class MeshFilterArgs(ctypes.Structure):
    """lr_mesh_filter_args, field for field.  out_n_vertices / out_n_faces are HOST long long."""
    _vp, _ll, _ci = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    _fields_ = [("struct_bytes", ctypes.c_size_t), ("n_vertices", _ll), ("n_faces", _ll), ("vertices", _vp), ("faces", _vp),
                ("colors", _vp), ("normals", _vp), ("keep_largest", _ci), ("min_faces", _ci), ("drop_degenerate", _ci),
                ("workspace", _vp), ("workspace_bytes", ctypes.c_size_t), ("out_n_vertices", _vp), ("out_n_faces", _vp),
                ("n_out_vertices", _ll), ("n_out_faces", _ll), ("out_vertices", _vp), ("out_colors", _vp), ("out_normals", _vp),
                ("out_faces", _vp), ("out_vertex_index", _vp), ("out_face_index", _vp), ("stream", _vp)]

    def __init__(self, **fields):
        super().__init__(struct_bytes=ctypes.sizeof(MeshFilterArgs), **fields)


class MeshNormalsArgs(ctypes.Structure):
    """lr_mesh_normals_args, field for field."""
    _vp, _ll = ctypes.c_void_p, ctypes.c_longlong
    _fields_ = [("struct_bytes", ctypes.c_size_t), ("n_vertices", _ll), ("n_faces", _ll), ("vertices", _vp), ("faces", _vp),
                ("out_normals", _vp), ("workspace", _vp), ("workspace_bytes", ctypes.c_size_t), ("stream", _vp)]

    def __init__(self, **fields):
        super().__init__(struct_bytes=ctypes.sizeof(MeshNormalsArgs), **fields)


LR_SCATTER_TILE = 256             # samples per on-chip tile of lr_scatter_interpolate (include/lucid_raster.h)


def assert_single_copy():
    """One library instance per process: raises if two DIFFERENT liblucid_raster.so files are mapped -- LR_LIB_DIR set without the
    same directory on LD_LIBRARY_PATH leaves the compiled binding on the default build while ctypes loads the other one: two sets of
    per-stream scratch, forward logs and tuning state, wrong answers from every query that crosses them, and (measured, round 6)
    a C3 step 1.5 % slower.  Called behind both loads (here and in _C.py); whichever comes second sees both."""
    try:
        with open("/proc/self/maps") as f:
            paths = {ln.split()[-1] for ln in f if ln.rstrip().endswith("liblucid_raster.so")}
    except OSError:                                                          # no procfs: nothing to check with
        return
    real = {os.path.realpath(p) for p in paths}
    if len(real) > 1:
        raise RuntimeError("luciddreamer_amd: two copies of liblucid_raster.so in this process (" + ", ".join(sorted(real)) +
                           "): LR_LIB_DIR needs the same directory on LD_LIBRARY_PATH (tools/diag_env.sh sets both)")


def lib():
    """Load the library (built by `python -m luciddreamer_amd.build` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"luciddreamer_amd: HIP library {LIB_PATH} is missing -- build it with "
                "`python -m luciddreamer_amd.build` (hipcc --offload-arch=gfx950). There is no CPU/PyTorch fallback.")
        L = ctypes.CDLL(LIB_PATH)
        assert_single_copy()
        vp, ci, cf, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
        L.lr_last_error.restype = ctypes.c_char_p
        L.lr_last_error.argtypes = []
        L.lr_version.restype = ctypes.c_char_p
        L.lr_version.argtypes = []
        L.lr_geom_bytes.restype = ctypes.c_size_t
        L.lr_geom_bytes.argtypes = [ci]
        L.lr_img_bytes.restype = ctypes.c_size_t
        L.lr_img_bytes.argtypes = [ci, ci]
        L.lr_binning_bytes.restype = ctypes.c_size_t
        L.lr_binning_bytes.argtypes = [ll]
        L.lr_forward.restype = ci
        L.lr_forward.argtypes = [ALLOC_FN, vp, ALLOC_FN, vp, ALLOC_FN, vp,      # allocators
                                 ci, ci, ci, vp, ci, ci,                         # P D M bg W H
                                 vp, vp, vp, vp, vp, cf, vp, vp,                 # means3D shs colors opac scales mod rot cov3D
                                 vp, vp, vp, cf, cf, ci,                         # view proj campos tanx tany prefiltered
                                 vp, vp, vp, ci, ll, vp]                         # out_color out_depth radii debug capacity stream
        L.lr_backward.restype = ci
        L.lr_backward.argtypes = [ci, ci, ci, ci, vp, ci, ci,                    # P D M R bg W H
                                  vp, vp, vp, vp, cf, vp, vp,                    # means3D shs colors scales mod rot cov3D
                                  vp, vp, vp, cf, cf, vp,                        # view proj campos tanx tany radii
                                  vp, vp, vp, vp, vp,                            # geom binning img dL_dpix dL_ddepth
                                  vp, vp, vp, vp, vp, vp, vp, vp, vp,            # 9 gradient outputs
                                  ci, ll, ctypes.c_uint, vp]                     # debug capacity accumulate_mask stream
        L.lr_view_forward.restype = ci
        L.lr_view_forward.argtypes = [ctypes.POINTER(ForwardArgs)]
        L.lr_view_backward.restype = ci
        L.lr_view_backward.argtypes = [ctypes.POINTER(BackwardArgs)]
        L.lr_render_alpha.restype = ci
        L.lr_render_alpha.argtypes = [vp, ci, ci, vp, vp]                        # image_buffer W H out_alpha stream
        L.lr_render_median.restype = ci
        L.lr_render_median.argtypes = [ctypes.POINTER(MedianArgs)]
        L.lr_median_backward.restype = ci
        L.lr_median_backward.argtypes = [ctypes.POINTER(MedianBackwardArgs)]
        L.lr_render_distortion.restype = ci
        L.lr_render_distortion.argtypes = [ctypes.POINTER(DistortionArgs)]
        L.lr_distortion_backward.restype = ci
        L.lr_distortion_backward.argtypes = [ctypes.POINTER(DistortionBackwardArgs)]
        L.lr_render_normals.restype = ci
        L.lr_render_normals.argtypes = [ctypes.POINTER(NormalsRenderArgs)]
        L.lr_render_normals_backward.restype = ci
        L.lr_render_normals_backward.argtypes = [ctypes.POINTER(NormalsRenderBackwardArgs)]
        L.lr_features_workspace_bytes.restype = ctypes.c_size_t
        L.lr_features_workspace_bytes.argtypes = [ll, ci]                        # slots channels
        L.lr_render_features.restype = ci
        L.lr_render_features.argtypes = [ctypes.POINTER(FeatureRenderArgs)]
        L.lr_render_features_backward.restype = ci
        L.lr_render_features_backward.argtypes = [ctypes.POINTER(FeatureRenderBackwardArgs)]
        L.lr_render_geometry.restype = ci
        L.lr_render_geometry.argtypes = [ctypes.POINTER(GeometryArgs)]
        L.lr_geometry_backward.restype = ci
        L.lr_geometry_backward.argtypes = [ctypes.POINTER(GeometryBackwardArgs)]
        L.lr_mark_visible.restype = ci
        L.lr_mark_visible.argtypes = [ci, vp, vp, vp, vp, vp]
        L.lr_check.restype = ci
        L.lr_check.argtypes = [vp, ctypes.POINTER(ll), vp]
        L.lr_dist2_workspace_bytes.restype = ctypes.c_size_t
        L.lr_dist2_workspace_bytes.argtypes = [ci]
        L.lr_dist2.restype = ci
        L.lr_dist2.argtypes = [ci, vp, vp, vp, vp]
        L.lr_dist2_workspace_layout.restype = ci
        L.lr_dist2_workspace_layout.argtypes = [ci, ctypes.POINTER(ctypes.c_size_t)]
        L.lr_views_workspace_bytes.restype = ctypes.c_size_t
        L.lr_views_workspace_bytes.argtypes = [ci, ci, ci, ll, ci, ctypes.c_uint]     # P W H capacity n_streams parts
        L.lr_views_accumulate.restype = ci
        L.lr_views_accumulate.argtypes = [ctypes.POINTER(ViewsArgs)]
        L.lr_views_check.restype = ci
        L.lr_views_check.argtypes = [vp, ci, ci, ci, ll, ci, ctypes.c_uint, vp]      # workspace, then as above, stream
        L.lr_depth_l1_workspace_bytes.restype = ctypes.c_size_t
        L.lr_depth_l1_workspace_bytes.argtypes = [ci, ci]
        L.lr_depth_l1_forward.restype = ci
        L.lr_depth_l1_forward.argtypes = [ci, ci, vp, vp, cf, vp, vp, ctypes.c_size_t, vp]
        L.lr_depth_l1_backward.restype = ci
        L.lr_depth_l1_backward.argtypes = [ci, ci, vp, vp, cf, vp, vp, vp]
        L.lr_depth_pearson_workspace_bytes.restype = ctypes.c_size_t
        L.lr_depth_pearson_workspace_bytes.argtypes = [ci, ci]
        L.lr_depth_pearson_forward.restype = ci
        L.lr_depth_pearson_forward.argtypes = [ci, ci, vp, vp, cf, vp, vp, ctypes.c_size_t, vp]
        L.lr_depth_pearson_backward.restype = ci
        L.lr_depth_pearson_backward.argtypes = [ci, ci, vp, vp, cf, vp, vp, ctypes.c_size_t, vp, vp]
        L.lr_masked_l1_dssim_forward.restype = ci
        L.lr_masked_l1_dssim_forward.argtypes = [ci, ci, ci, vp, vp, vp, cf, vp, vp, ctypes.c_size_t, vp]
        L.lr_masked_l1_dssim_backward.restype = ci
        L.lr_masked_l1_dssim_backward.argtypes = [ci, ci, ci, vp, vp, vp, cf, vp, vp, vp, vp]
        L.lr_alpha_hole_workspace_bytes.restype = ctypes.c_size_t
        L.lr_alpha_hole_workspace_bytes.argtypes = [ci, ci]
        L.lr_alpha_hole_forward.restype = ci
        L.lr_alpha_hole_forward.argtypes = [ci, ci, vp, vp, cf, vp, vp, ctypes.c_size_t, vp]
        L.lr_alpha_hole_backward.restype = ci
        L.lr_alpha_hole_backward.argtypes = [ci, ci, vp, cf, vp, vp, vp]
        L.lr_video_workspace_bytes.restype = ctypes.c_size_t
        L.lr_video_workspace_bytes.argtypes = [ci, ci, ci]
        L.lr_frames_to_u8.restype = ci
        L.lr_frames_to_u8.argtypes = [ci, ci, ci, vp, vp, vp]
        L.lr_depth_colorize.restype = ci
        L.lr_depth_colorize.argtypes = [ci, ci, ci, vp, ci, cf,                  # n H W depths from_render invalid_val
                                        cf, cf, vp, vp, ci,                      # q_lo q_hi fixed_vmin_vmax lut lut_n
                                        ctypes.c_char_p, vp, vp,                 # background (host, 4 bytes) out_rgba out_vmin_vmax
                                        vp, ctypes.c_size_t, vp]                 # workspace bytes stream
        L.lr_loss_workspace_bytes.restype = ctypes.c_size_t
        L.lr_loss_workspace_bytes.argtypes = [ci, ci, ci]
        L.lr_l1_dssim_forward.restype = ci
        L.lr_l1_dssim_forward.argtypes = [ci, ci, ci, vp, vp, cf, vp, vp, ctypes.c_size_t, vp]
        L.lr_l1_dssim_backward.restype = ci
        L.lr_l1_dssim_backward.argtypes = [ci, ci, ci, vp, vp, cf, vp, vp, vp, vp]
        L.lr_l1_dssim_backward_weights.restype = ci
        L.lr_l1_dssim_backward_weights.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
        L.lr_select_workspace_bytes.restype = ctypes.c_size_t
        L.lr_select_workspace_bytes.argtypes = [ci]
        L.lr_select_rows.restype = ci
        L.lr_select_rows.argtypes = [ci, vp, ci, vp, vp, vp, ll, vp, vp, ctypes.c_size_t, vp]
        L.lr_pack_ply_rows.restype = ci
        L.lr_pack_ply_rows.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]
        L.lr_densify_stats.restype = ci
        L.lr_densify_stats.argtypes = [ci, vp, vp, vp, vp, vp, vp]
        L.lr_adam_step.restype = ci
        cd = ctypes.c_double
        L.lr_adam_step.argtypes = [ci, vp, vp, vp, vp, vp, vp, cd, cd, cd, ci, vp]
        L.lr_mcmc_workspace_bytes.restype = ctypes.c_size_t
        L.lr_mcmc_workspace_bytes.argtypes = [ci, ci]
        L.lr_mcmc_relocate.restype = ci
        L.lr_mcmc_relocate.argtypes = [ctypes.POINTER(McmcRelocateArgs)]
        L.lr_mcmc_noise.restype = ci
        L.lr_mcmc_noise.argtypes = [ci, vp, vp, vp, vp, vp, cf, vp]              # P xyz scale rotation opacity noise scaler stream
        L.lr_mcmc_reg_grad.restype = ci
        L.lr_mcmc_reg_grad.argtypes = [ci, vp, vp, cf, cf, vp, vp, vp]           # P opacity scale w_opacity w_scale dL_do dL_ds stream
        L.lr_filter3d_workspace_bytes.restype = ctypes.c_size_t
        L.lr_filter3d_workspace_bytes.argtypes = [ci]
        L.lr_filter3d_update.restype = ci
        L.lr_filter3d_update.argtypes = [ci, ci, vp, vp, cf, vp, vp, vp, vp]     # P V means3D cams variance filter seen workspace stream
        L.lr_filter3d_apply_forward.restype = ci
        L.lr_filter3d_apply_forward.argtypes = [ci, vp, vp, vp, ci, vp, vp, vp]  # P scale opacity filter activated out_scale out_opacity stream
        L.lr_filter3d_apply_backward.restype = ci
        L.lr_filter3d_apply_backward.argtypes = [ci, vp, vp, vp, ci, vp, vp, vp, vp, vp]   # ... g_scale g_opacity d_scale d_opacity stream
        L.lr_reproject_workspace_bytes.restype = ctypes.c_size_t
        L.lr_reproject_workspace_bytes.argtypes = [ci, ci, ci]
        L.lr_reproject.restype = ci
        L.lr_reproject.argtypes = [ctypes.POINTER(ReprojectArgs)]
        L.lr_lift.restype = ci
        L.lr_lift.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp]                   # H W depth Kinv Rinv RinvT (host) out stream
        L.lr_dream_workspace_bytes.restype = ctypes.c_size_t
        L.lr_dream_workspace_bytes.argtypes = [ll]
        for fn in (L.lr_dream_scale_sums, L.lr_dream_correspond, L.lr_dream_lift):
            fn.restype = ci
            fn.argtypes = [ctypes.POINTER(DreamArgs)]
        L.lr_scatter_interpolate.restype = ci
        L.lr_scatter_interpolate.argtypes = [ctypes.POINTER(ScatterArgs)]
        L.lr_normals_workspace_bytes.restype = ctypes.c_size_t
        L.lr_normals_workspace_bytes.argtypes = [ci, ci]
        for fn in (L.lr_depth_normals, L.lr_depth_normals_backward, L.lr_normal_loss_forward, L.lr_normal_loss_backward):
            fn.restype = ci
            fn.argtypes = [ctypes.POINTER(NormalsArgs)]
        L.lr_smooth_workspace_bytes.restype = ctypes.c_size_t
        L.lr_smooth_workspace_bytes.argtypes = [ci, ci]
        for fn in (L.lr_smooth_forward, L.lr_smooth_backward):
            fn.restype = ci
            fn.argtypes = [ctypes.POINTER(SmoothArgs)]
        L.lr_tsdf_workspace_bytes.restype = ctypes.c_size_t
        L.lr_tsdf_workspace_bytes.argtypes = [ctypes.POINTER(TsdfExtractArgs)]
        L.lr_tsdf_integrate.restype = ci
        L.lr_tsdf_integrate.argtypes = [ctypes.POINTER(TsdfIntegrateArgs)]
        for fn in (L.lr_tsdf_extract_count, L.lr_tsdf_extract_emit):
            fn.restype = ci
            fn.argtypes = [ctypes.POINTER(TsdfExtractArgs)]
        L.lr_mesh_workspace_bytes.restype = ctypes.c_size_t
        L.lr_mesh_workspace_bytes.argtypes = [ll, ll]
        L.lr_mesh_components.restype = ci
        L.lr_mesh_components.argtypes = [ctypes.POINTER(MeshComponentsArgs)]
        for fn in (L.lr_mesh_filter_count, L.lr_mesh_filter_emit):
            fn.restype = ci
            fn.argtypes = [ctypes.POINTER(MeshFilterArgs)]
        L.lr_mesh_vertex_normals.restype = ci
        L.lr_mesh_vertex_normals.argtypes = [ctypes.POINTER(MeshNormalsArgs)]
        L.lr_step_begin.restype = ci
        L.lr_step_begin.argtypes = []
        L.lr_step_end.restype = ci
        L.lr_step_end.argtypes = [vp]
        L.lr_step_abort.restype = ci
        L.lr_step_abort.argtypes = []
        L.lr_forward_ticket.restype = ctypes.c_longlong
        L.lr_forward_ticket.argtypes = []
        L.lr_tune_set.restype = ci
        L.lr_tune_set.argtypes = [ctypes.c_char_p, ci]
        L.lr_set_antialiasing.restype = ci
        L.lr_set_antialiasing.argtypes = [ci]
        L.lr_get_antialiasing.restype = ci
        L.lr_get_antialiasing.argtypes = []
        L.lr_last_launch_shapes.restype = ci
        L.lr_last_launch_shapes.argtypes = [ctypes.POINTER(ci), ctypes.POINTER(ci)]
        L.lr_last_forward_channels.restype = ci
        L.lr_last_forward_channels.argtypes = [ctypes.POINTER(ci)]
        L.lr_profile_enable.restype = ci
        L.lr_profile_enable.argtypes = [ci]
        L.lr_profile_stage_name.restype = ctypes.c_char_p
        L.lr_profile_stage_name.argtypes = [ci]
        L.lr_profile_read.restype = ci
        L.lr_profile_read.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ll), ci]
        _lib = L
    return _lib


class _NoGuard:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def on_device(dev):
    """`with on_device(dev):` -- make `dev` the current HIP device for the C call inside.  When it already is (the one-GPU case:
    every call of a training loop) this is a shared no-op object instead of torch.cuda.device's save / set / restore, ~8 us of
    host time per call on paths whose host time is what a LucidDreamer-sized iteration lasts."""
    import torch
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    return _NO_GUARD if torch.cuda.current_device() == idx else torch.cuda.device(dev)


def tune_set(name, value):
    """Test hook: force one of the shipped code paths (lr_tune_set); value -1 restores the library's own rule.  Values that
    select a retired kernel raise unless the diagnostics build is loaded (diagnostics_build())."""
    rc = lib().lr_tune_set(name.encode(), int(value))
    if rc < 0:
        raise RuntimeError(last_error())


def diagnostics_build():
    """True when the loaded library was compiled with -DLR_DIAGNOSTICS (retired kernels, LR_* environment overrides)."""
    return b"+diagnostics" in lib().lr_version()


FWD_SHAPES = {-1: None, 0: "quadrant", 1: "quadrant-pairs", 2: "tile"}
BWD_SHAPES = {-1: None, 0: "half", 1: "quad", 2: "tile"}


def last_launch_shapes():
    """(forward, backward) kernel shapes of the process's last blend launches (lr_last_launch_shapes)."""
    f, b = ctypes.c_int(-1), ctypes.c_int(-1)
    lib().lr_last_launch_shapes(ctypes.byref(f), ctypes.byref(b))
    return FWD_SHAPES.get(f.value, f.value), BWD_SHAPES.get(b.value, b.value)


FWD_CHANNELS = {-1: None, 0: "none", 1: "color", 3: "color+depth"}


def last_forward_channels():
    """Channel set of the process's last blend forward (lr_last_forward_channels): "color+depth", "color", or "none" for the
    colour-free forward of a multi-view step driven by fixed gradients."""
    c = ctypes.c_int(-1)
    lib().lr_last_forward_channels(ctypes.byref(c))
    return FWD_CHANNELS.get(c.value, c.value)


def profile_enable(on=True):
    """Start (clearing previous records) or stop per-stage HIP-event timing inside the library."""
    return lib().lr_profile_enable(1 if on else 0)


def profile_read():
    """{stage: (total_ms, calls)} for everything recorded since profile_enable(True); waits for the events."""
    L = lib()
    n = 16                                   # >= number of stages (lr_profile_read returns the real count)
    ms = (ctypes.c_double * n)()
    calls = (ctypes.c_longlong * n)()
    cnt = L.lr_profile_read(ms, calls, n)
    if cnt < 0:
        raise RuntimeError(last_error())
    return {L.lr_profile_stage_name(i).decode(): (ms[i], int(calls[i])) for i in range(cnt)}


def last_error():
    return lib().lr_last_error().decode("utf-8", "replace")


def raise_for(code, where):
    """Map a negative return code to the exception type the reference raises."""
    msg = last_error()
    if code == LR_ERR_INVALID_ARG:
        raise RuntimeError(f"{where}: {msg}")
    if code == LR_ERR_PREFILTERED:
        raise RuntimeError(msg)
    if code == LR_ERR_OVERFLOW:
        raise RuntimeError(f"{where}: {msg}")
    raise RuntimeError(f"{where}: error {code}: {msg}")
