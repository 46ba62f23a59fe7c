"""ctypes binding of include/vips_hip.h (libvips_amd/lib/libvipship.so).

Plumbing only: every signature here is the C ABI's, nothing is computed in
Python.  The library is built by ``__graft_entry__.build()`` (hipcc, gfx950).
There is no CPU fallback: if the shared library is missing, import fails loudly.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# VIPS_HIP_LIBRARY: load another build of the same library (e.g. a sanitizer build, tools/asan_mock.sh)
LIB_PATH = os.environ.get("VIPS_HIP_LIBRARY") or os.path.join(_HERE, "lib", "libvipship.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "vips_hip.h")


class VipsHipError(RuntimeError):
    """Mirrors libvips' error convention: -1 + a message in the error buffer."""


class Region(ctypes.Structure):
    """VipsHipRegion (include/vips_hip.h)."""

    _fields_ = [
        ("data", ctypes.c_void_p),
        ("left", ctypes.c_int),
        ("top", ctypes.c_int),
        ("width", ctypes.c_int),
        ("height", ctypes.c_int),
        ("im_width", ctypes.c_int),
        ("im_height", ctypes.c_int),
        ("bands", ctypes.c_int),
        ("format", ctypes.c_int),
        ("stride", ctypes.c_size_t),
    ]


class VHeader(ctypes.Structure):
    """VipsHipVHeader: the fields of a .v file header (include/vips_hip.h)."""

    _fields_ = [
        ("width", ctypes.c_int),
        ("height", ctypes.c_int),
        ("bands", ctypes.c_int),
        ("format", ctypes.c_int),
        ("coding", ctypes.c_int),
        ("interpretation", ctypes.c_int),
        ("xres", ctypes.c_float),
        ("yres", ctypes.c_float),
        ("xoffset", ctypes.c_int),
        ("yoffset", ctypes.c_int),
        ("msb_first", ctypes.c_int),
        ("data_offset", ctypes.c_longlong),
        ("data_size", ctypes.c_longlong),
    ]


class JpegHeader(ctypes.Structure):
    """VipsHipJpegHeader (include/vips_hip.h)."""

    _fields_ = [
        ("width", ctypes.c_int),
        ("height", ctypes.c_int),
        ("bands", ctypes.c_int),
        ("interpretation", ctypes.c_int),
        ("image_width", ctypes.c_int),
        ("image_height", ctypes.c_int),
        ("orientation", ctypes.c_int),
        ("has_icc", ctypes.c_int),
    ]


class Affine(ctypes.Structure):
    """VipsHipAffine (include/vips_hip.h): the arguments of vips_affine."""

    MAX_BACKGROUND = 64
    _fields_ = [
        ("a", ctypes.c_double), ("b", ctypes.c_double), ("c", ctypes.c_double), ("d", ctypes.c_double),
        ("odx", ctypes.c_double), ("ody", ctypes.c_double), ("idx", ctypes.c_double), ("idy", ctypes.c_double),
        ("oarea", ctypes.c_int * 4),
        ("have_oarea", ctypes.c_int),
        ("interpolate", ctypes.c_int),
        ("extend", ctypes.c_int),
        ("premultiplied", ctypes.c_int),
        ("force_tiles", ctypes.c_int),
        ("n_background", ctypes.c_int),
        ("background", ctypes.c_double * 64),
    ]


class Mapim(ctypes.Structure):
    """VipsHipMapim (include/vips_hip.h): the optional arguments of vips_mapim."""

    MAX_BACKGROUND = 64
    _fields_ = [
        ("interpolate", ctypes.c_int),
        ("extend", ctypes.c_int),
        ("premultiplied", ctypes.c_int),
        ("n_background", ctypes.c_int),
        ("background", ctypes.c_double * 64),
    ]


class Embed(ctypes.Structure):
    """VipsHipEmbed (include/vips_hip.h): the optional arguments of vips_embed / vips_gravity."""

    MAX_BACKGROUND = 32
    _fields_ = [
        ("extend", ctypes.c_int),
        ("extend_set", ctypes.c_int),
        ("n_background", ctypes.c_int),
        ("background", ctypes.c_double * 32),
    ]


class Flatten(ctypes.Structure):
    """VipsHipFlatten (include/vips_hip.h)."""

    _fields_ = [
        ("n_background", ctypes.c_int),
        ("background", ctypes.c_double * 32),
        ("max_alpha_set", ctypes.c_int),
        ("max_alpha", ctypes.c_double),
    ]


class Insert(ctypes.Structure):
    """VipsHipInsert (include/vips_hip.h): the optional arguments of vips_insert / vips_join."""

    _fields_ = [
        ("expand", ctypes.c_int),
        ("n_background", ctypes.c_int),
        ("background", ctypes.c_double * 32),
        ("shim", ctypes.c_int),
        ("align", ctypes.c_int),
    ]


class Arrayjoin(ctypes.Structure):
    """VipsHipArrayjoin (include/vips_hip.h): the optional arguments of vips_arrayjoin."""

    MAX_BACKGROUND = 32
    _fields_ = [
        ("across", ctypes.c_int),
        ("shim", ctypes.c_int),
        ("n_background", ctypes.c_int),
        ("background", ctypes.c_double * 32),
        ("halign", ctypes.c_int),
        ("valign", ctypes.c_int),
        ("hspacing", ctypes.c_int),
        ("vspacing", ctypes.c_int),
    ]


class Linear(ctypes.Structure):
    """VipsHipLinear (include/vips_hip.h): the arguments of vips_linear."""

    MAX_VECTOR = 32
    _fields_ = [
        ("n_a", ctypes.c_int),
        ("a", ctypes.c_double * 32),
        ("n_b", ctypes.c_int),
        ("b", ctypes.c_double * 32),
        ("uchar", ctypes.c_int),
    ]


class FindTrim(ctypes.Structure):
    """VipsHipFindTrim (include/vips_hip.h): the optional arguments of vips_find_trim."""

    MAX_BACKGROUND = 32
    _fields_ = [
        ("threshold", ctypes.c_double),
        ("n_background", ctypes.c_int),
        ("background", ctypes.c_double * 32),
        ("line_art", ctypes.c_int),
    ]


def _load():
    # PyTorch-ROCm carries its own HIP runtime (soname libamdhip64.so).  Import it first so
    # libvipship.so, which needs that soname, binds to the SAME runtime: device pointers,
    # streams and events can then be shared with torch, and there is one runtime at exit.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the HIP extension is the product; there is no fallback path)" % LIB_PATH
        )
    return ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)


lib = _load()

c_int, c_double, c_void_p, c_size_t, c_char_p = (
    ctypes.c_int,
    ctypes.c_double,
    ctypes.c_void_p,
    ctypes.c_size_t,
    ctypes.c_char_p,
)
P = ctypes.POINTER
RegionP = P(Region)

_SIGNATURES = {
    # runtime
    "vips_hip_init": (c_int, [c_int]),
    "vips_hip_shutdown": (None, []),
    "vips_hip_device_count": (c_int, []),
    "vips_hip_current_device": (c_int, []),
    "vips_hip_devices": (c_int, [P(c_int), c_int]),
    "vips_hip_error_buffer": (c_char_p, []),
    "vips_hip_error_clear": (None, []),
    "vips_hip_set_stream": (c_int, [c_void_p]),
    "vips_hip_get_stream": (c_void_p, []),
    "vips_hip_synchronize": (c_int, []),
    "vips_hip_malloc": (c_void_p, [c_size_t]),
    "vips_hip_free": (None, [c_void_p]),
    "vips_hip_malloc_host": (c_void_p, [c_size_t]),
    "vips_hip_free_host": (None, [c_void_p]),
    "vips_hip_memcpy_h2d": (c_int, [c_void_p, c_void_p, c_size_t]),
    "vips_hip_memcpy_d2h": (c_int, [c_void_p, c_void_p, c_size_t]),
    "vips_hip_memcpy_h2d_async": (c_int, [c_void_p, c_void_p, c_size_t]),
    "vips_hip_memcpy_d2h_async": (c_int, [c_void_p, c_void_p, c_size_t]),
    "vips_hip_stream_new": (c_void_p, []),
    "vips_hip_stream_free": (None, [c_void_p]),
    "vips_hip_event_synchronize": (c_int, [c_void_p]),
    "vips_hip_stream_wait_event": (c_int, [c_void_p]),
    "vips_hip_memcpy_d2d": (c_int, [c_void_p, c_void_p, c_size_t]),
    "vips_hip_memcpy2d_h2d": (c_int, [c_void_p, c_size_t, c_void_p, c_size_t, c_size_t, c_size_t]),
    "vips_hip_memcpy2d_d2h": (c_int, [c_void_p, c_size_t, c_void_p, c_size_t, c_size_t, c_size_t]),
    "vips_hip_pool_bytes": (c_size_t, []),
    "vips_hip_pool_trim": (None, []),
    "vips_hip_event_new": (c_void_p, []),
    "vips_hip_event_free": (None, [c_void_p]),
    "vips_hip_event_record": (c_int, [c_void_p]),
    "vips_hip_event_elapsed_ms": (c_double, [c_void_p, c_void_p]),
    "vips_hip_gate_enable": (None, [c_int]),
    "vips_hip_gate_reset": (None, []),
    "vips_hip_gate_query": (c_int, [c_char_p, P(c_double)]),
    "vips_hip_gate_report": (c_int, [c_char_p, c_int]),
    # reduce
    "vips_hip_reduce_new": (c_void_p, [c_int, c_double, c_int, c_int, c_double]),
    "vips_hip_reduce_free": (None, [c_void_p]),
    "vips_hip_reduce_get_n_point": (c_int, [c_void_p]),
    "vips_hip_reduce_get_out_size": (c_int, [c_void_p]),
    "vips_hip_reduce_get_offset": (c_double, [c_void_p]),
    "vips_hip_reduce_get_matrixs": (c_int, [c_void_p, c_int, P(ctypes.c_short)]),
    "vips_hip_reduce_get_matrixf": (c_int, [c_void_p, c_int, P(c_double)]),
    "vips_hip_reduce_get_points": (c_int, [c_int, c_double]),
    "vips_hip_reduceh_need": (None, [c_void_p, c_int, c_int, P(c_int), P(c_int)]),
    "vips_hip_reducev_need": (None, [c_void_p, c_int, c_int, P(c_int), P(c_int)]),
    "vips_hip_reduceh_gen": (c_int, [c_void_p, RegionP, RegionP]),
    "vips_hip_reducev_gen": (c_int, [c_void_p, RegionP, RegionP]),
    "vips_hip_reduceh_gen_tiled": (c_int, [c_void_p, RegionP, RegionP, c_int]),
    "vips_hip_reducev_gen_tiled": (c_int, [c_void_p, RegionP, RegionP, c_int]),
    "vips_hip_upsize_gen": (c_int, [RegionP, RegionP, c_double, c_double, c_double, c_double, c_int, c_int]),
    "vips_hip_affine_out_size": (c_int, [c_int, c_double]),
    "vips_hip_zoom_gen": (c_int, [RegionP, RegionP, c_int, c_int]),
    "vips_hip_subsample_gen": (c_int, [RegionP, RegionP, c_int, c_int]),
    "vips_hip_upsize_step": (c_int, [c_int]),
    "vips_hip_reduce_gen": (c_int, [c_void_p, c_void_p, RegionP, RegionP]),
    "vips_hip_reduce_gen_tiled": (c_int, [c_void_p, c_void_p, RegionP, RegionP, c_int]),
    # shrink
    "vips_hip_shrinkh_gen": (c_int, [c_int, RegionP, RegionP]),
    "vips_hip_shrinkv_gen": (c_int, [c_int, RegionP, RegionP]),
    "vips_hip_shrink_out_size": (c_int, [c_int, c_int, c_int]),
    # convolution
    "vips_hip_conv_new": (c_void_p, [P(c_double), c_int, c_int, c_double, c_double, c_int]),
    "vips_hip_conv_free": (None, [c_void_p]),
    "vips_hip_conv_get_nnz": (c_int, [c_void_p]),
    "vips_hip_conv_get_vector": (c_int, [c_void_p, P(c_int), P(c_int), P(c_int), c_int]),
    "vips_hip_conv_out_format": (c_int, [c_void_p, c_int]),
    "vips_hip_conv_gen": (c_int, [c_void_p, RegionP, RegionP]),
    "vips_hip_conv_step": (c_int, [c_int]),
    "vips_hip_conva_step": (c_int, [c_int]),
    "vips_hip_vector_set_enabled": (None, [c_int]),
    "vips_hip_vector_isenabled": (c_int, []),
    "vips_hip_set_exact_float": (None, [c_int]),
    "vips_hip_get_exact_float": (c_int, []),
    "vips_hip_conva_new": (c_void_p, [P(c_double), c_int, c_int, c_double, c_double, c_int, c_int]),
    "vips_hip_convasep_new": (c_void_p, [P(c_double), c_int, c_double, c_double, c_int]),
    "vips_hip_conva_free": (None, [c_void_p]),
    "vips_hip_conva_get_lines": (c_int, [c_void_p, P(c_int), P(c_int), c_int]),
    "vips_hip_conva_gen": (c_int, [c_void_p, RegionP, RegionP]),
    "vips_hip_convasep_gen": (c_int, [c_void_p, RegionP, RegionP, c_int]),
    "vips_hip_gaussmat": (c_int, [c_double, c_double, c_int, c_int, P(c_double), c_int, P(c_double)]),
    # colour
    "vips_hip_colour_gen": (c_int, [c_int, RegionP, RegionP]),
    "vips_hip_colour_route_gen": (c_int, [P(c_int), c_int, c_double, RegionP, RegionP]),
    "vips_hip_cast_gen": (c_int, [RegionP, RegionP]),
    "vips_hip_premultiply_gen": (c_int, [RegionP, RegionP, c_double, c_int, c_int]),
    "vips_hip_sharpen_gen": (c_int, [c_void_p, RegionP, RegionP, RegionP]),
    # images
    "vips_hip_image_new": (c_void_p, [c_int, c_int, c_int, c_int, c_int]),
    "vips_hip_image_new_from_memory": (c_void_p, [c_void_p, c_int, c_int, c_int, c_int, c_int]),
    "vips_hip_image_new_from_device": (c_void_p, [c_void_p, c_int, c_int, c_int, c_int, c_int]),
    "vips_hip_image_unref": (None, [c_void_p]),
    "vips_hip_image_unref_many": (None, [P(c_void_p), c_int]),
    "vips_hip_image_write_to_memory": (c_int, [c_void_p, c_void_p]),
    "vips_hip_image_get_data": (c_void_p, [c_void_p]),
    "vips_hip_image_get_device": (c_int, [c_void_p]),
    "vips_hip_image_get_width": (c_int, [c_void_p]),
    "vips_hip_image_get_height": (c_int, [c_void_p]),
    "vips_hip_image_get_bands": (c_int, [c_void_p]),
    "vips_hip_image_get_format": (c_int, [c_void_p]),
    "vips_hip_image_get_interpretation": (c_int, [c_void_p]),
    "vips_hip_image_get_stride": (c_size_t, [c_void_p]),
    "vips_hip_image_region": (None, [c_void_p, RegionP]),
    "vips_hip_set_fatstrip_height": (None, [c_int]),
    # operations
    "vips_hip_reduceh": (c_int, [c_void_p, P(c_void_p), c_double, c_int, c_double]),
    "vips_hip_reducev": (c_int, [c_void_p, P(c_void_p), c_double, c_int, c_double]),
    "vips_hip_reduce": (c_int, [c_void_p, P(c_void_p), c_double, c_double, c_int, c_double]),
    "vips_hip_shrinkh": (c_int, [c_void_p, P(c_void_p), c_int, c_int]),
    "vips_hip_shrinkv": (c_int, [c_void_p, P(c_void_p), c_int, c_int]),
    "vips_hip_shrink": (c_int, [c_void_p, P(c_void_p), c_double, c_double, c_int]),
    "vips_hip_resize": (c_int, [c_void_p, P(c_void_p), c_double, c_double, c_int, c_double]),
    "vips_hip_thumbnail_image": (c_int, [c_void_p, P(c_void_p), c_int, c_int, c_int, c_int]),
    "vips_hip_conv": (c_int, [c_void_p, P(c_void_p), P(c_double), c_int, c_int, c_double, c_double, c_int]),
    "vips_hip_convsep": (c_int, [c_void_p, P(c_void_p), P(c_double), c_int, c_double, c_double, c_int]),
    "vips_hip_vfile_read_header": (c_int, [c_char_p, P(VHeader)]),
    "vips_hip_image_new_from_vfile": (c_void_p, [c_char_p]),
    "vips_hip_image_write_to_vfile": (c_int, [c_void_p, c_char_p]),
    "vips_hip_thumbnail_find_jpegshrink": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "vips_hip_jpeg_read_header": (c_int, [c_char_p, c_int, P(JpegHeader)]),
    "vips_hip_jpeg_read_to_memory": (c_int, [c_char_p, c_int, c_void_p, c_size_t]),
    "vips_hip_image_new_from_jpeg": (c_void_p, [c_char_p, c_int]),
    "vips_hip_thumbnail": (c_int, [c_char_p, P(c_void_p), c_int, c_int, c_int, c_int, c_int]),
    "vips_hip_thumbnail_batch": (c_int, [P(c_char_p), c_int, P(c_void_p), c_char_p, c_int, c_int, c_int, c_int,
                                         c_int, c_int]),
    "vips_hip_thumbnail_image_crop": (c_int, [c_void_p, P(c_void_p), c_int, c_int, c_int, c_int, c_int]),
    "vips_hip_extract_area": (c_int, [c_void_p, P(c_void_p), c_int, c_int, c_int, c_int]),
    "vips_hip_conva": (c_int, [c_void_p, P(c_void_p), P(c_double), c_int, c_int, c_double, c_double, c_int, c_int]),
    "vips_hip_convasep": (c_int, [c_void_p, P(c_void_p), P(c_double), c_int, c_double, c_double, c_int]),
    "vips_hip_gaussblur": (c_int, [c_void_p, P(c_void_p), c_double, c_double, c_int]),
    "vips_hip_sharpen": (c_int, [c_void_p, P(c_void_p), c_double, c_double, c_double, c_double, c_double, c_double]),
    "vips_hip_colourspace": (c_int, [c_void_p, P(c_void_p), c_int]),
    "vips_hip_strips_new": (c_void_p, [c_int, c_int, c_int, c_int, c_int, P(c_int), c_int]),
    "vips_hip_strips_free": (None, [c_void_p]),
    "vips_hip_strips_count": (c_int, [c_void_p]),
    "vips_hip_strips_region": (c_int, [c_void_p, c_int, P(c_int), P(Region), P(Region)]),
    "vips_hip_strips_exchange": (c_int, [c_void_p]),
    "vips_hip_conv_strips": (c_int, [c_void_p, P(c_void_p), P(c_double), c_int, c_int, c_double, c_double, c_int]),
    "vips_hip_resize_sharpen_batch": (c_int, [P(c_void_p), c_int, P(c_void_p), c_double, c_int, c_double,
                                             c_double, c_double, c_double, c_double, c_double, c_double, c_int]),
    "vips_hip_resize_sharpen_batch_queue": (c_int, [P(c_void_p), c_int, P(c_void_p), c_double, c_int, c_double,
                                             c_double, c_double, c_double, c_double, c_double, c_double, c_int]),
    "vips_hip_gaussblur_colourspace": (c_int, [c_void_p, P(c_void_p), c_double, c_double, c_int, c_int]),
    "vips_hip_cast": (c_int, [c_void_p, P(c_void_p), c_int]),
    # rot / flip / autorot, the orientation
    "vips_hip_rot_gen": (c_int, [c_int, RegionP, RegionP]),
    "vips_hip_flip_gen": (c_int, [c_int, RegionP, RegionP]),
    "vips_hip_rot_tile_side": (c_int, [c_int]),
    "vips_hip_rot_step": (c_int, [c_int]),
    "vips_hip_rot_group": (c_int, [c_int]),
    "vips_hip_rot": (c_int, [c_void_p, P(c_void_p), c_int]),
    "vips_hip_flip": (c_int, [c_void_p, P(c_void_p), c_int]),
    "vips_hip_autorot": (c_int, [c_void_p, P(c_void_p), P(c_int), P(c_int)]),
    "vips_hip_image_get_orientation": (c_int, [c_void_p]),
    "vips_hip_image_set_orientation": (c_int, [c_void_p, c_int]),
    "vips_hip_vfile_read_orientation": (c_int, [c_char_p, P(c_int)]),
    "vips_hip_thumbnail_find_jpegshrink_rotate": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "vips_hip_thumbnail_image_rotate": (c_int, [c_void_p, P(c_void_p), c_int, c_int, c_int, c_int, c_int, c_int]),
    "vips_hip_thumbnail_rotate": (c_int, [c_char_p, P(c_void_p), c_int, c_int, c_int, c_int, c_int, c_int]),
    "vips_hip_thumbnail_batch_rotate": (c_int, [P(c_char_p), c_int, P(c_void_p), c_char_p, c_int, c_int, c_int,
                                                c_int, c_int, c_int, c_int]),
    # histograms, smartcrop
    "vips_hip_hist_find": (c_int, [c_void_p, P(c_void_p), c_int]),
    "vips_hip_hist_rects": (c_int, [c_void_p, P(c_int), c_int, P(ctypes.c_uint)]),
    "vips_hip_hist_step": (c_int, [c_int]),
    "vips_hip_smartcrop": (c_int, [c_void_p, P(c_void_p), c_int, c_int, c_int, P(c_int), P(c_int), P(c_int), P(c_int)]),
    # maplut, hist_cum / hist_norm / hist_equal, hist_local, stdif
    "vips_hip_maplut": (c_int, [c_void_p, c_void_p, P(c_void_p), c_int]),
    "vips_hip_hist_cum": (c_int, [c_void_p, P(c_void_p)]),
    "vips_hip_hist_norm": (c_int, [c_void_p, P(c_void_p)]),
    "vips_hip_hist_cum_host": (None, [P(ctypes.c_uint), c_int, c_int, P(ctypes.c_uint)]),
    "vips_hip_hist_norm_host": (c_int, [P(ctypes.c_uint), c_int, c_int, c_void_p]),
    "vips_hip_hist_equal": (c_int, [c_void_p, P(c_void_p), c_int]),
    "vips_hip_hist_local_gen": (c_int, [RegionP, RegionP, c_int, c_int, c_int]),
    "vips_hip_hist_local_step": (c_int, [c_int]),
    "vips_hip_hist_local": (c_int, [c_void_p, P(c_void_p), c_int, c_int, c_int]),
    "vips_hip_stdif_gen": (c_int, [RegionP, RegionP, c_int, c_int, c_double, c_double, c_double, c_double]),
    "vips_hip_stdif_step": (c_int, [c_int]),
    "vips_hip_stdif": (c_int, [c_void_p, P(c_void_p), c_int, c_int, c_double, c_double, c_double, c_double]),
    # rank / median / morph
    "vips_hip_rank_gen": (c_int, [RegionP, RegionP, c_int, c_int, c_int]),
    "vips_hip_morph_gen": (c_int, [RegionP, RegionP, P(c_double), c_int, c_int, c_int]),
    "vips_hip_rank_need": (None, [c_int, c_int, c_int, P(c_int), P(c_int)]),
    "vips_hip_rank_step": (c_int, [c_int]),
    "vips_hip_rank": (c_int, [c_void_p, P(c_void_p), c_int, c_int, c_int]),
    "vips_hip_median": (c_int, [c_void_p, P(c_void_p), c_int]),
    "vips_hip_morph": (c_int, [c_void_p, P(c_void_p), P(c_double), c_int, c_int, c_int]),
    # sobel / scharr / prewitt
    "vips_hip_edge_gen": (c_int, [RegionP, RegionP, c_int]),
    "vips_hip_edge_need": (None, [c_int, c_int, P(c_int), P(c_int)]),
    "vips_hip_edge_step": (c_int, [c_int]),
    "vips_hip_sobel": (c_int, [c_void_p, P(c_void_p)]),
    "vips_hip_scharr": (c_int, [c_void_p, P(c_void_p)]),
    "vips_hip_prewitt": (c_int, [c_void_p, P(c_void_p)]),
    # canny
    "vips_hip_canny_table": (None, [P(ctypes.c_ubyte)]),
    "vips_hip_canny_need": (None, [c_int, c_int, P(c_int), P(c_int)]),
    "vips_hip_canny_gen": (c_int, [RegionP, RegionP]),
    "vips_hip_canny_marginal": (ctypes.c_longlong, []),
    "vips_hip_canny": (c_int, [c_void_p, P(c_void_p), c_double, c_int]),
    # compass
    "vips_hip_rot45": (c_int, [P(c_double), c_int, c_int, c_int, P(c_double)]),
    "vips_hip_compass_new": (c_void_p, [P(c_double), c_int, c_int, c_double, c_double, c_int, c_int, c_int, c_int, c_int,
                                        c_int]),
    "vips_hip_compass_free": (None, [c_void_p]),
    "vips_hip_compass_get_masks": (c_int, [c_void_p, P(c_double), P(c_int), c_int]),
    "vips_hip_compass_out_format": (c_int, [c_void_p, c_int]),
    "vips_hip_compass_gen": (c_int, [c_void_p, RegionP, RegionP]),
    "vips_hip_compass": (c_int, [c_void_p, P(c_void_p), P(c_double), c_int, c_int, c_double, c_double, c_int, c_int, c_int,
                                 c_int, c_int, c_int]),
    "vips_hip_premultiply": (c_int, [c_void_p, P(c_void_p), c_int]),
    "vips_hip_unpremultiply": (c_int, [c_void_p, P(c_void_p), c_int]),
    # affine / similarity / rotate
    "vips_hip_affine_defaults": (None, [P(Affine)]),
    "vips_hip_affine_plan_new": (c_void_p, [P(Affine), c_int, c_int, c_int, c_int, c_int]),
    "vips_hip_affine_plan_free": (None, [c_void_p]),
    "vips_hip_affine_plan_get": (c_int, [c_void_p, c_int]),
    "vips_hip_affine_need": (None, [c_void_p, c_int, c_int, c_int, c_int, P(c_int)]),
    "vips_hip_affine_gen": (c_int, [c_void_p, RegionP, RegionP, c_int]),
    "vips_hip_affine": (c_int, [c_void_p, P(c_void_p), P(Affine)]),
    "vips_hip_similarity": (c_int, [c_void_p, P(c_void_p), c_double, c_double, P(Affine)]),
    "vips_hip_rotate": (c_int, [c_void_p, P(c_void_p), c_double, P(Affine)]),
    # mapim, xyz
    "vips_hip_mapim_defaults": (None, [P(Mapim)]),
    "vips_hip_mapim": (c_int, [c_void_p, c_void_p, P(c_void_p), P(Mapim)]),
    "vips_hip_mapim_need": (c_int, [RegionP, P(Mapim), c_int, c_int, P(c_int)]),
    "vips_hip_mapim_bounds_need": (c_int, [P(c_double), P(Mapim), c_int, c_int, P(c_int)]),
    "vips_hip_mapim_gen": (c_int, [RegionP, RegionP, RegionP, P(Mapim), c_int, c_int]),
    "vips_hip_mapim_step": (c_int, [c_int]),
    "vips_hip_xyz": (c_int, [P(c_void_p), c_int, c_int]),
    # fastcor, spcor
    "vips_hip_fastcor": (c_int, [c_void_p, c_void_p, P(c_void_p)]),
    "vips_hip_spcor": (c_int, [c_void_p, c_void_p, P(c_void_p)]),
    "vips_hip_spcor_constants": (c_int, [c_void_p, c_int, c_int, c_int, c_int, ctypes.c_size_t, c_int, P(c_double), P(c_double)]),
    "vips_hip_correlation_step": (c_int, [c_int]),
    # embed / gravity / insert / join, flatten, addalpha
    "vips_hip_embed_defaults": (None, [P(Embed)]),
    "vips_hip_flatten_defaults": (None, [P(Flatten)]),
    "vips_hip_insert_defaults": (None, [P(Insert)]),
    "vips_hip_vector_to_ink": (c_int, [P(c_double), c_int, c_int, c_int, c_void_p]),
    "vips_hip_embed_plan": (c_int, [c_char_p, P(Embed), c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                    P(c_int), P(c_int), c_void_p]),
    "vips_hip_gravity_position": (c_int, [c_int, c_int, c_int, c_int, c_int, P(c_int), P(c_int)]),
    "vips_hip_embed_need": (None, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P(c_int)]),
    "vips_hip_embed_gen": (c_int, [c_int, c_void_p, c_int, c_int, RegionP, RegionP]),
    "vips_hip_flatten_gen": (c_int, [RegionP, RegionP, c_double, c_int, c_void_p]),
    "vips_hip_embed": (c_int, [c_void_p, P(c_void_p), c_int, c_int, c_int, c_int, P(Embed)]),
    "vips_hip_gravity": (c_int, [c_void_p, P(c_void_p), c_int, c_int, c_int, P(Embed)]),
    "vips_hip_flatten": (c_int, [c_void_p, P(c_void_p), P(Flatten)]),
    "vips_hip_addalpha": (c_int, [c_void_p, P(c_void_p)]),
    "vips_hip_insert": (c_int, [c_void_p, c_void_p, P(c_void_p), c_int, c_int, P(Insert)]),
    "vips_hip_join": (c_int, [c_void_p, c_void_p, P(c_void_p), c_int, P(Insert)]),
    "vips_hip_canvas_step": (c_int, [c_int, c_int]),
    # arrayjoin / replicate / wrap / grid, zoom / subsample
    "vips_hip_arrayjoin_defaults": (None, [P(Arrayjoin)]),
    "vips_hip_arrayjoin_plan": (c_int, [P(Arrayjoin), c_int, P(c_int), P(c_int), P(c_int), P(c_int), P(c_int), P(c_int), P(c_int)]),
    "vips_hip_arrayjoin": (c_int, [P(c_void_p), c_int, P(c_void_p), P(Arrayjoin)]),
    "vips_hip_replicate": (c_int, [c_void_p, P(c_void_p), c_int, c_int]),
    "vips_hip_wrap": (c_int, [c_void_p, P(c_void_p), c_int, c_int, c_int, c_int]),
    "vips_hip_grid": (c_int, [c_void_p, P(c_void_p), c_int, c_int, c_int]),
    "vips_hip_replicate_need": (None, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P(c_int)]),
    "vips_hip_grid_need": (None, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P(c_int)]),
    "vips_hip_replicate_gen": (c_int, [c_int, c_int, RegionP, RegionP]),
    "vips_hip_grid_gen": (c_int, [c_int, c_int, RegionP, RegionP]),
    "vips_hip_zoom": (c_int, [c_void_p, P(c_void_p), c_int, c_int]),
    "vips_hip_subsample": (c_int, [c_void_p, P(c_void_p), c_int, c_int]),
    "vips_hip_cells_step": (c_int, [c_int, c_int]),
    # linear / invert / abs, add / subtract / multiply / divide, stats / avg / deviate / min / max
    "vips_hip_linear_defaults": (None, [P(Linear)]),
    "vips_hip_arith_format": (c_int, [c_int, c_int]),
    "vips_hip_linear_plan": (c_int, [P(Linear), c_int, c_int, P(c_int), P(c_int), P(c_int), P(c_double), P(c_double)]),
    "vips_hip_binary_plan": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                     P(c_int), P(c_int), P(c_int), P(c_int), P(c_int), P(c_int)]),
    "vips_hip_stats_finish": (c_int, [P(c_double), c_int, ctypes.c_longlong]),
    "vips_hip_linear_gen": (c_int, [P(Linear), RegionP, RegionP]),
    "vips_hip_invert_gen": (c_int, [RegionP, RegionP]),
    "vips_hip_abs_gen": (c_int, [RegionP, RegionP]),
    "vips_hip_linear": (c_int, [c_void_p, P(c_void_p), P(Linear)]),
    "vips_hip_invert": (c_int, [c_void_p, P(c_void_p)]),
    "vips_hip_abs": (c_int, [c_void_p, P(c_void_p)]),
    "vips_hip_add": (c_int, [c_void_p, c_void_p, P(c_void_p)]),
    "vips_hip_subtract": (c_int, [c_void_p, c_void_p, P(c_void_p)]),
    "vips_hip_multiply": (c_int, [c_void_p, c_void_p, P(c_void_p)]),
    "vips_hip_divide": (c_int, [c_void_p, c_void_p, P(c_void_p)]),
    "vips_hip_round_gen": (c_int, [c_int, RegionP, RegionP]),
    "vips_hip_sign_gen": (c_int, [RegionP, RegionP]),
    "vips_hip_clamp_gen": (c_int, [c_double, c_double, RegionP, RegionP]),
    "vips_hip_remainder_const_gen": (c_int, [P(c_double), c_int, RegionP, RegionP]),
    "vips_hip_round": (c_int, [c_void_p, P(c_void_p), c_int]),
    "vips_hip_sign": (c_int, [c_void_p, P(c_void_p)]),
    "vips_hip_clamp": (c_int, [c_void_p, P(c_void_p), c_double, c_double]),
    "vips_hip_remainder_const": (c_int, [c_void_p, P(c_void_p), P(c_double), c_int]),
    "vips_hip_minpair": (c_int, [c_void_p, c_void_p, P(c_void_p)]),
    "vips_hip_maxpair": (c_int, [c_void_p, c_void_p, P(c_void_p)]),
    "vips_hip_remainder": (c_int, [c_void_p, c_void_p, P(c_void_p)]),
    "vips_hip_recomb_plan": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, P(c_int), P(c_int)]),
    "vips_hip_recomb_gen": (c_int, [P(c_double), c_int, c_int, RegionP, RegionP]),
    "vips_hip_recomb_matrix": (c_int, [c_void_p, P(c_void_p), P(c_double), c_int, c_int]),
    "vips_hip_recomb": (c_int, [c_void_p, P(c_void_p), c_void_p]),
    "vips_hip_recomb_step": (c_int, [c_int]),
    "vips_hip_nary_plan": (c_int, [c_int, c_int] + [P(c_int)] * 5 + [c_int] + [P(c_int)] * 7),
    "vips_hip_sum": (c_int, [P(c_void_p), c_int, P(c_void_p)]),
    "vips_hip_bandrank": (c_int, [P(c_void_p), c_int, P(c_void_p), c_int]),
    "vips_hip_nary_step": (c_int, [c_int]),
    "vips_hip_stats": (c_int, [c_void_p, P(c_double)]),
    "vips_hip_avg": (c_int, [c_void_p, P(c_double)]),
    "vips_hip_deviate": (c_int, [c_void_p, P(c_double)]),
    "vips_hip_min": (c_int, [c_void_p, P(c_double), P(c_int), P(c_int)]),
    "vips_hip_max": (c_int, [c_void_p, P(c_double), P(c_int), P(c_int)]),
    "vips_hip_arith_step": (c_int, [c_int]),
    # relational / boolean, ifthenelse, bandjoin / extract_band / bandmean / bandbool
    "vips_hip_logic_format": (c_int, [c_int, c_int]),
    "vips_hip_const_plan": (c_int, [ctypes.c_char_p, P(c_double), c_int, c_int, c_int, P(c_int), P(c_int), P(c_int), P(c_double)]),
    "vips_hip_logic_plan": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                    P(c_int), P(c_int), P(c_int), P(c_int), P(c_int), P(c_int)]),
    "vips_hip_ifthenelse_plan": (c_int, [c_int] * 15 + [P(c_int)] * 5),
    "vips_hip_bandjoin_plan": (c_int, [c_int, P(c_int), P(c_int), P(c_int), P(c_int), c_int] + [P(c_int)] * 5),
    "vips_hip_relational_const_gen": (c_int, [c_int, P(c_double), c_int, RegionP, RegionP]),
    "vips_hip_boolean_const_gen": (c_int, [c_int, P(c_double), c_int, RegionP, RegionP]),
    "vips_hip_bandjoin_const_gen": (c_int, [P(c_double), c_int, RegionP, RegionP]),
    "vips_hip_extract_band_gen": (c_int, [c_int, RegionP, RegionP]),
    "vips_hip_bandmean_gen": (c_int, [RegionP, RegionP]),
    "vips_hip_bandbool_gen": (c_int, [c_int, RegionP, RegionP]),
    "vips_hip_relational_const": (c_int, [c_void_p, P(c_void_p), c_int, P(c_double), c_int]),
    "vips_hip_boolean_const": (c_int, [c_void_p, P(c_void_p), c_int, P(c_double), c_int]),
    "vips_hip_relational": (c_int, [c_void_p, c_void_p, P(c_void_p), c_int]),
    "vips_hip_boolean": (c_int, [c_void_p, c_void_p, P(c_void_p), c_int]),
    "vips_hip_ifthenelse": (c_int, [c_void_p, c_void_p, c_void_p, P(c_void_p), c_int]),
    "vips_hip_bandjoin": (c_int, [P(c_void_p), c_int, P(c_void_p)]),
    "vips_hip_bandjoin_const": (c_int, [c_void_p, P(c_void_p), P(c_double), c_int]),
    "vips_hip_extract_band": (c_int, [c_void_p, P(c_void_p), c_int, c_int]),
    "vips_hip_bandmean": (c_int, [c_void_p, P(c_void_p)]),
    "vips_hip_bandbool": (c_int, [c_void_p, P(c_void_p), c_int]),
    "vips_hip_logic_step": (c_int, [c_int]),
    # project / profile / getpoint / find_trim
    "vips_hip_project_format": (c_int, [c_int]),
    "vips_hip_project": (c_int, [c_void_p, P(c_void_p), P(c_void_p)]),
    "vips_hip_profile": (c_int, [c_void_p, P(c_void_p), P(c_void_p)]),
    "vips_hip_getpoint": (c_int, [c_void_p, c_int, c_int, P(c_double), c_int]),
    "vips_hip_find_trim_defaults": (None, [P(FindTrim)]),
    "vips_hip_find_trim_background": (c_double, [c_int]),
    "vips_hip_find_trim_finish": (c_int, [P(ctypes.c_uint), c_int, P(ctypes.c_uint), c_int] + [P(c_int)] * 4),
    "vips_hip_find_trim_table": (c_int, [P(FindTrim), c_int, c_int, P(c_int), P(ctypes.c_ubyte)]),
    "vips_hip_find_trim": (c_int, [c_void_p, P(FindTrim)] + [P(c_int)] * 4),
    "vips_hip_trim_step": (c_int, [c_int]),
    # labelregions / countlines
    "vips_hip_labelregions": (c_int, [c_void_p, P(c_void_p), P(c_int)]),
    "vips_hip_labelregions_step": (c_int, [c_int]),
    "vips_hip_countlines": (c_int, [c_void_p, c_int, P(c_double)]),
    "vips_hip_countlines_step": (c_int, [c_int]),
}

MISSING = []
for _name, (_res, _args) in _SIGNATURES.items():
    try:
        _fn = getattr(lib, _name)
    except AttributeError:
        MISSING.append(_name)
        continue
    _fn.restype = _res
    _fn.argtypes = _args


def error_buffer():
    return lib.vips_hip_error_buffer().decode("utf-8", "replace")


def _raise(what):
    message = error_buffer().strip() or what
    lib.vips_hip_error_clear()
    raise VipsHipError(message)


def check(result, what="vips_hip"):
    """Turn the C convention (non-zero return + error buffer) into an exception."""
    if result != 0:
        _raise(what)
    return result


def check_handle(handle, what="vips_hip"):
    """NULL handle + error buffer -> exception."""
    if not handle:
        _raise(what)
    return handle
