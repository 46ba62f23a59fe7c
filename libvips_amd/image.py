"""Host-side mirror of the reference's image API for the hot path.

``Image`` wraps a device-resident ``VipsHipImage`` and exposes the operations
with the names / argument meaning / error behaviour of the reference's Python
binding (pyvips, which the reference's own test-suite uses:
test/test-suite/test_resample.py, test_convolution.py, test_colour.py), so the
parity tests read like the reference's tests.  Every method is a single call
through the C ABI (include/vips_hip.h); no pixel is touched in Python.
"""
import ctypes
import os

import numpy as np

from . import _ffi
from ._ffi import lib, check, check_handle

# VipsBandFormat (include/vips/image.h:120-133)
FORMATS = {
    "uchar": 0,
    "char": 1,
    "ushort": 2,
    "short": 3,
    "uint": 4,
    "int": 5,
    "float": 6,
    "complex": 7,
    "double": 8,
    "dpcomplex": 9,
}
FORMAT_NAMES = {v: k for k, v in FORMATS.items()}
FORMAT_DTYPES = {
    0: np.uint8,
    1: np.int8,
    2: np.uint16,
    3: np.int16,
    4: np.uint32,
    5: np.int32,
    6: np.float32,
    7: np.complex64,
    8: np.float64,
    9: np.complex128,
}
DTYPE_FORMATS = {np.dtype(v): k for k, v in FORMAT_DTYPES.items()}

# VipsKernel (include/vips/resample.h:41-51)
KERNELS = {
    "nearest": 0,
    "linear": 1,
    "cubic": 2,
    "mitchell": 3,
    "lanczos2": 4,
    "lanczos3": 5,
    "mks2013": 6,
    "mks2021": 7,
}
# VipsPrecision (include/vips/basic.h:106-110)
PRECISIONS = {"integer": 0, "float": 1, "approximate": 2}
# VipsSize (include/vips/resample.h), VipsInteresting (include/vips/conversion.h:97-107)
SIZES = {"both": 0, "up": 1, "down": 2, "force": 3}
INTERESTING = {"none": 0, "centre": 1, "entropy": 2, "attention": 3, "low": 4, "high": 5, "all": 6}
# VipsAngle, VipsDirection (include/vips/conversion.h)
ANGLES = {"d0": 0, "d90": 1, "d180": 2, "d270": 3}
ANGLE_NAMES = {v: k for k, v in ANGLES.items()}
DIRECTIONS = {"horizontal": 0, "vertical": 1}
# VipsOperationMorphology (include/vips/morphology.h)
MORPHOLOGIES = {"erode": 0, "dilate": 1}
ANGLES45 = {"d0": 0, "d45": 1, "d90": 2, "d135": 3, "d180": 4, "d225": 5, "d270": 6, "d315": 7}
COMBINES = {"max": 0, "sum": 1, "min": 2}
# VipsExtend (include/vips/conversion.h); the interpolators the device has (resample/interpolate.c, bicubic.cpp)
EXTENDS = {"black": 0, "copy": 1, "repeat": 2, "mirror": 3, "white": 4, "background": 5}
INTERPOLATORS = {"nearest": 0, "bilinear": 1, "bicubic": 2}
# VipsCompassDirection, VipsAlign (include/vips/conversion.h)
COMPASS_DIRECTIONS = {"centre": 0, "north": 1, "east": 2, "south": 3, "west": 4, "north-east": 5, "south-east": 6,
                      "south-west": 7, "north-west": 8}
ALIGNS = {"low": 0, "centre": 1, "high": 2}
# VipsInterpretation (include/vips/image.h:94-118)
INTERPRETATIONS = {
    "multiband": 0,
    "b-w": 1,
    "histogram": 10,
    "xyz": 12,
    "lab": 13,
    "labs": 21,
    "srgb": 22,
    "rgb16": 25,
    "grey16": 26,
    "scrgb": 28,
}
INTERPRETATION_NAMES = {v: k for k, v in INTERPRETATIONS.items()}


def _enum(table, value, what):
    if isinstance(value, str):
        try:
            return table[value.lower()]
        except KeyError:
            raise ValueError("unknown %s %r" % (what, value))
    return int(value)


def _guess_interpretation(bands, fmt):
    # vips_image_new_from_memory defaults (iofuncs/image.c): multiband; the
    # reference's tests set interpretation explicitly via copy().
    return 0


class Image(object):
    """A device-resident image (VipsHipImage)."""

    def __init__(self, handle, keepalive=None):
        check_handle(handle, "image")
        self._h = ctypes.c_void_p(handle)
        self._keepalive = keepalive

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            lib.vips_hip_image_unref(h)
            self._h = None

    # ------------------------------------------------------------ creation
    @classmethod
    def new_from_array(cls, array, interpretation="multiband"):
        """Upload a (height, width[, bands]) numpy array."""
        a = np.ascontiguousarray(array)
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3:
            raise ValueError("need a 2D or 3D array")
        fmt = DTYPE_FORMATS[a.dtype]
        h, w, b = a.shape
        handle = lib.vips_hip_image_new_from_memory(
            a.ctypes.data, w, h, b, fmt, _enum(INTERPRETATIONS, interpretation, "interpretation")
        )
        return cls(check_handle(handle))

    @classmethod
    def new_from_file(cls, path):
        """Load a libvips native .v file into HBM (iofuncs/vips.c; pinned double-buffered upload)."""
        return cls(check_handle(lib.vips_hip_image_new_from_vfile(os.fsencode(path))))

    def write_to_file(self, path):
        """Save as a libvips native .v file."""
        check(lib.vips_hip_image_write_to_vfile(self._h, os.fsencode(path)))

    @classmethod
    def new_from_tensor(cls, tensor, interpretation="multiband"):
        """Wrap (no copy) a contiguous (H, W, C) torch CUDA tensor."""
        import torch

        if not tensor.is_cuda or not tensor.is_contiguous():
            raise ValueError("need a contiguous CUDA tensor")
        # The library's own streams are non-blocking: work torch has queued on the tensor
        # (fills, copies) must be complete before a kernel on another stream reads it.
        cur = torch.cuda.current_stream(tensor.device)
        if (lib.vips_hip_get_stream() or 0) != cur.cuda_stream:
            cur.synchronize()
        t = tensor if tensor.dim() == 3 else tensor.unsqueeze(-1)
        np_dtype = np.dtype(str(t.dtype).replace("torch.", ""))
        fmt = DTYPE_FORMATS[np_dtype]
        h, w, b = t.shape
        handle = lib.vips_hip_image_new_from_device(
            t.data_ptr(), w, h, b, fmt, _enum(INTERPRETATIONS, interpretation, "interpretation")
        )
        return cls(check_handle(handle), keepalive=tensor)

    @classmethod
    def new_from_device(cls, ptr, width, height, bands, format, interpretation="multiband", keepalive=None):
        handle = lib.vips_hip_image_new_from_device(
            ptr, width, height, bands, _enum(FORMATS, format, "format"),
            _enum(INTERPRETATIONS, interpretation, "interpretation"),
        )
        return cls(check_handle(handle), keepalive=keepalive)

    # ---------------------------------------------------------- properties
    @property
    def width(self):
        return lib.vips_hip_image_get_width(self._h)

    @property
    def height(self):
        return lib.vips_hip_image_get_height(self._h)

    @property
    def bands(self):
        return lib.vips_hip_image_get_bands(self._h)

    @property
    def format(self):
        return FORMAT_NAMES[lib.vips_hip_image_get_format(self._h)]

    @property
    def interpretation(self):
        v = lib.vips_hip_image_get_interpretation(self._h)
        return INTERPRETATION_NAMES.get(v, v)

    @property
    def orientation(self):
        """The EXIF-style orientation, 1 .. 8 (an image without one reads as 1, as in pyvips); ``has_orientation``
        tells the two apart.  Set by the JPEG and .v loaders, kept by rot / flip, undone by autorot."""
        return lib.vips_hip_image_get_orientation(self._h) or 1

    @orientation.setter
    def orientation(self, value):
        check(lib.vips_hip_image_set_orientation(self._h, int(value) if value else 0))

    @property
    def has_orientation(self):
        return lib.vips_hip_image_get_orientation(self._h) != 0

    @property
    def data_ptr(self):
        return lib.vips_hip_image_get_data(self._h)

    def region(self):
        r = _ffi.Region()
        lib.vips_hip_image_region(self._h, ctypes.byref(r))
        return r

    def numpy(self):
        """Download: vips_image_write_to_memory (iofuncs/image.c:2901)."""
        fmt = lib.vips_hip_image_get_format(self._h)
        out = np.empty((self.height, self.width, self.bands), dtype=FORMAT_DTYPES[fmt])
        check(lib.vips_hip_image_write_to_memory(self._h, out.ctypes.data))
        return out

    # ---------------------------------------------------------- operations
    def _unary(self, fn, *args):
        out = ctypes.c_void_p()
        check(fn(self._h, ctypes.byref(out), *args))
        return Image(out.value)

    def reduceh(self, hshrink, kernel="lanczos3", gap=0.0):
        return self._unary(lib.vips_hip_reduceh, float(hshrink), _enum(KERNELS, kernel, "kernel"), float(gap))

    def reducev(self, vshrink, kernel="lanczos3", gap=0.0):
        return self._unary(lib.vips_hip_reducev, float(vshrink), _enum(KERNELS, kernel, "kernel"), float(gap))

    def reduce(self, hshrink, vshrink, kernel="lanczos3", gap=0.0):
        return self._unary(
            lib.vips_hip_reduce, float(hshrink), float(vshrink), _enum(KERNELS, kernel, "kernel"), float(gap)
        )

    def shrinkh(self, hshrink, ceil=False):
        return self._unary(lib.vips_hip_shrinkh, int(hshrink), int(bool(ceil)))

    def shrinkv(self, vshrink, ceil=False):
        return self._unary(lib.vips_hip_shrinkv, int(vshrink), int(bool(ceil)))

    def shrink(self, hshrink, vshrink, ceil=False):
        return self._unary(lib.vips_hip_shrink, float(hshrink), float(vshrink), int(bool(ceil)))

    def resize(self, scale, vscale=None, kernel="lanczos3", gap=2.0):
        return self._unary(
            lib.vips_hip_resize,
            float(scale),
            float(vscale) if vscale is not None else -1.0,
            _enum(KERNELS, kernel, "kernel"),
            float(gap),
        )

    @classmethod
    def new_from_jpeg(cls, path, shrink=1):
        """jpegload with shrink-on-load 1/2/4/8 (foreign/jpeg2vips.c): host decode, upload."""
        return cls(check_handle(lib.vips_hip_image_new_from_jpeg(os.fsencode(path), int(shrink))))

    @classmethod
    def thumbnail(cls, path, width, height=None, size="both", linear=False, crop="none", no_rotate=None):
        """vips_thumbnail() for JPEG and .v files: shrink-on-load, then the thumbnail_image pipeline.
        ``no_rotate=False`` undoes the file's orientation as vips_thumbnail does by default, ``True`` keeps the
        pixels as stored and the tag on the result; ``None`` is the entry point without auto-rotation, which refuses
        an oriented JPEG."""
        out = ctypes.c_void_p()
        args = (os.fsencode(path), ctypes.byref(out), int(width), int(height) if height else 0,
                _enum(SIZES, size, "size"), int(bool(linear)), _enum(INTERESTING, crop, "crop"))
        if no_rotate is None:
            check(lib.vips_hip_thumbnail(*args))
        else:
            check(lib.vips_hip_thumbnail_rotate(*args, int(bool(no_rotate))))
        return cls(out.value)

    @classmethod
    def thumbnail_batch(cls, paths, width, height=None, size="both", linear=False, crop="none", threads=8,
                        no_rotate=None):
        """vips_thumbnail() over many files on `threads` host threads (decode and device work of
        different files overlap).  Returns a list of Images; a failed file gives a VipsHipError
        instance in its place."""
        from ._ffi import VipsHipError

        n = len(paths)
        arr = (ctypes.c_char_p * n)(*[os.fsencode(p) for p in paths])
        outs = (ctypes.c_void_p * n)()
        errors = ctypes.create_string_buffer(256 * max(n, 1))
        args = (arr, n, outs, errors, int(width), int(height) if height else 0, _enum(SIZES, size, "size"),
                int(bool(linear)), _enum(INTERESTING, crop, "crop"))
        if no_rotate is None:
            r = lib.vips_hip_thumbnail_batch(*args, int(threads))
        else:
            r = lib.vips_hip_thumbnail_batch_rotate(*args, int(bool(no_rotate)), int(threads))
        if r < 0:
            check(r)
        result = []
        for i in range(n):
            if outs[i]:
                result.append(cls(outs[i]))
            else:
                result.append(VipsHipError(errors.raw[256 * i:256 * i + 256].split(b"\0", 1)[0].decode()))
        return result

    def thumbnail_image(self, width, height=None, size="both", linear=False, crop="none", no_rotate=None):
        args = (int(width), int(height) if height else 0, _enum(SIZES, size, "size"), int(bool(linear)),
                _enum(INTERESTING, crop, "crop"))
        if no_rotate is None:  # the entry point that does not look at the orientation
            return self._unary(lib.vips_hip_thumbnail_image_crop, *args)
        return self._unary(lib.vips_hip_thumbnail_image_rotate, *args, int(bool(no_rotate)))

    # vips_rot / vips_flip / vips_autorot, with pyvips' names
    def rot(self, angle):
        return self._unary(lib.vips_hip_rot, _enum(ANGLES, angle, "angle"))

    def rot90(self):
        return self.rot("d90")

    def rot180(self):
        return self.rot("d180")

    def rot270(self):
        return self.rot("d270")

    def flip(self, direction):
        return self._unary(lib.vips_hip_flip, _enum(DIRECTIONS, direction, "direction"))

    def fliphor(self):
        return self.flip("horizontal")

    def flipver(self):
        return self.flip("vertical")

    def autorot(self, with_options=False):
        """Undo the orientation (one launch for a turn plus a flip); the result has none.  ``with_options``: also
        return ``{"angle": "d90", "flip": False}``, the operation's optional outputs."""
        angle, flip = ctypes.c_int(), ctypes.c_int()
        out = self._unary(lib.vips_hip_autorot, ctypes.byref(angle), ctypes.byref(flip))
        if with_options:
            return out, {"angle": ANGLE_NAMES[angle.value], "flip": bool(flip.value)}
        return out

    def extract_area(self, left, top, width, height):
        return self._unary(lib.vips_hip_extract_area, int(left), int(top), int(width), int(height))

    crop = extract_area

    def hist_find(self, band=-1):
        """vips_hist_find of a uchar image: a uint image one row high, as wide as the largest counted value + 1
        (256 when every band is counted), of interpretation histogram."""
        return self._unary(lib.vips_hip_hist_find, int(band))

    def hist_rects(self, rects):
        """The histograms of up to six (left, top, width, height) rectangles in one launch of the histogram kernel:
        an (n, 256, bands) uint32 array."""
        n = len(rects)
        flat = (ctypes.c_int * (4 * max(n, 1)))(*[int(v) for r in rects for v in r])
        out = np.zeros((n, 256, self.bands), np.uint32)
        check(lib.vips_hip_hist_rects(self._h, flat, n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint))))
        return out

    # libvips/histogram: vips_hist_cum / vips_hist_norm / vips_hist_equal / vips_maplut / vips_hist_local / vips_stdif
    def hist_cum(self):
        """The cumulative histogram of a one-row uint histogram (what hist_find makes), band by band."""
        return self._unary(lib.vips_hip_hist_cum)

    def hist_norm(self):
        """vips_hist_norm of a one-row uint histogram: every band scaled so that its maximum is width - 1, in the
        smallest unsigned format that holds it (uchar for the 256 entries of a uchar image)."""
        return self._unary(lib.vips_hip_hist_norm)

    def hist_equal(self, band=-1):
        """Global histogram equalisation of a uchar image: every band through its own cumulative histogram, or
        (``band=k``) every band through band k's."""
        return self._unary(lib.vips_hip_hist_equal, int(band))

    def maplut(self, lut, band=-1):
        """out = lut[in] for a uchar image: ``lut`` is an Image one row or column of up to 256 entries, of any
        non-complex format, of one band, this image's bands, or any bands when this image has one.  ``band=k`` with a
        one-band LUT maps band k only.  The result has the LUT's format."""
        out = ctypes.c_void_p()
        check(lib.vips_hip_maplut(self._h, lut._h, ctypes.byref(out), int(band)))
        return Image(out.value)

    def hist_local(self, width, height, max_slope=0):
        """Local histogram equalisation over ``width`` x ``height`` windows (uchar, edges mirrored); ``max_slope`` 1
        .. 100 limits the contrast gain (CLAHE)."""
        return self._unary(lib.vips_hip_hist_local, int(width), int(height), int(max_slope))

    def stdif(self, width, height, a=0.5, m0=128.0, b=0.5, s0=50.0):
        """Statistical differencing over ``width`` x ``height`` windows (uchar, edges copied): pull the local mean
        towards ``m0`` (weight ``a``) and the local deviation towards ``s0`` (weight ``b``)."""
        return self._unary(lib.vips_hip_stdif, int(width), int(height), float(a), float(m0), float(b), float(s0))

    def smartcrop(self, width, height, interesting="attention", with_options=False):
        """vips_smartcrop.  ``with_options``: also return ``{"left", "top", "attention_x", "attention_y"}``: where
        the crop was taken and, for the attention mode, the point it found."""
        left, top, ax, ay = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        out = self._unary(lib.vips_hip_smartcrop, int(width), int(height), _enum(INTERESTING, interesting, "interesting"),
                          ctypes.byref(left), ctypes.byref(top), ctypes.byref(ax), ctypes.byref(ay))
        if with_options:
            return out, {"left": left.value, "top": top.value, "attention_x": ax.value, "attention_y": ay.value}
        return out

    # vips_rank / vips_median / vips_morph
    def rank(self, width, height, index):
        """The ``index``-th smallest (from 0) of every ``width`` x ``height`` window, band by band, edges copied."""
        return self._unary(lib.vips_hip_rank, int(width), int(height), int(index))

    def median(self, size=3):
        return self._unary(lib.vips_hip_median, int(size))

    def morph(self, mask, morph):
        """Erode or dilate by a mask (a nested list or array) of 0, 128 and 255; the result is uchar."""
        m = self._mask(mask)
        return self._unary(lib.vips_hip_morph, m.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), m.shape[1], m.shape[0],
                           _enum(MORPHOLOGIES, morph, "morph"))

    # vips_sobel / vips_scharr / vips_prewitt: the result is uchar
    def sobel(self):
        return self._unary(lib.vips_hip_sobel)

    def scharr(self):
        return self._unary(lib.vips_hip_scharr)

    def prewitt(self):
        return self._unary(lib.vips_hip_prewitt)

    def canny(self, sigma=1.4, precision="float"):
        """vips_canny: blur, gradient, polar image and thinning.  uchar for a uchar image with precision integer or
        approximate, else float.  ``libvips_amd.canny_marginal()`` says how many pels of the float path sat too close
        to a rounding boundary of theta to be sure of."""
        return self._unary(lib.vips_hip_canny, float(sigma), _enum(PRECISIONS, precision, "precision"))

    def compass(self, mask, times=2, angle="d90", combine="max", precision="float", layers=5, cluster=1, scale=1.0,
                offset=0.0):
        """vips_compass: convolve ``times`` times, the (odd, square) mask turned by ``angle`` in between, and combine
        the absolute values.  max and min keep the convolution's format, sum widens it as vips_sum does."""
        m = self._mask(mask)
        return self._unary(lib.vips_hip_compass, m.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), m.shape[1], m.shape[0],
                           float(scale), float(offset), int(times), _enum(ANGLES45, angle, "angle"),
                           _enum(COMBINES, combine, "combine"), _enum(PRECISIONS, precision, "precision"), int(layers),
                           int(cluster))

    @staticmethod
    def _mask(mask):
        m = np.ascontiguousarray(np.asarray(mask, dtype=np.float64))
        if m.ndim == 1:
            m = m[None, :]
        return m

    # vips_affine / vips_similarity / vips_rotate, with pyvips' argument names
    @staticmethod
    def affine_args(matrix=(1, 0, 0, 1), interpolate="bilinear", oarea=None, odx=0, ody=0, idx=0, idy=0, background=None,
                    extend="background", premultiplied=False):
        """The VipsHipAffine of these arguments (also what vips_hip_affine_plan_new takes)."""
        args = _ffi.Affine()
        lib.vips_hip_affine_defaults(ctypes.byref(args))
        args.a, args.b, args.c, args.d = [float(v) for v in matrix]
        if isinstance(interpolate, str) and interpolate.lower() not in INTERPOLATORS:
            raise _ffi.VipsHipError("affine: interpolator %s is outside the HIP path (nearest, bilinear, bicubic)"
                                    % interpolate)
        args.interpolate = _enum(INTERPOLATORS, interpolate, "interpolate")
        if oarea is not None:
            if len(oarea) != 4:
                raise _ffi.VipsHipError("affine: vector must have 4 elements")
            args.oarea[:] = [int(v) for v in oarea]
            args.have_oarea = 1
        args.odx, args.ody, args.idx, args.idy = float(odx), float(ody), float(idx), float(idy)
        if background is not None:
            background = [float(v) for v in np.atleast_1d(background)]
            if len(background) > _ffi.Affine.MAX_BACKGROUND:
                raise _ffi.VipsHipError("affine: background of more than %d elements" % _ffi.Affine.MAX_BACKGROUND)
            args.n_background = len(background)
            args.background[:len(background)] = background
        args.extend = _enum(EXTENDS, extend, "extend")
        args.premultiplied = int(bool(premultiplied))
        return args

    def affine(self, matrix, **kwargs):
        """vips_affine: ``matrix`` is (a, b, c, d); interpolate "nearest" / "bilinear" / "bicubic", ``oarea`` (left,
        top, width, height), odx, ody, idx, idy, background, extend and premultiplied as in pyvips."""
        return self._unary(lib.vips_hip_affine, ctypes.byref(self.affine_args(matrix, **kwargs)))

    def similarity(self, scale=1.0, angle=0.0, **kwargs):
        return self._unary(lib.vips_hip_similarity, float(scale), float(angle), ctypes.byref(self.affine_args(**kwargs)))

    def rotate(self, angle, **kwargs):
        return self._unary(lib.vips_hip_rotate, float(angle), ctypes.byref(self.affine_args(**kwargs)))

    # vips_mapim and vips_xyz, with pyvips' argument names
    @staticmethod
    def mapim_args(interpolate="bilinear", extend="background", background=0, premultiplied=False):
        """The VipsHipMapim of these arguments."""
        args = _ffi.Mapim()
        lib.vips_hip_mapim_defaults(ctypes.byref(args))
        if isinstance(interpolate, str) and interpolate.lower() not in INTERPOLATORS:
            raise _ffi.VipsHipError("mapim: interpolator %s is outside the HIP path (nearest, bilinear, bicubic)"
                                    % interpolate)
        args.interpolate = _enum(INTERPOLATORS, interpolate, "interpolate")
        args.extend = _enum(EXTENDS, extend, "extend")
        if background is not None:
            background = [float(v) for v in np.atleast_1d(background)]
            if len(background) > _ffi.Mapim.MAX_BACKGROUND:
                raise _ffi.VipsHipError("mapim: background of more than %d elements" % _ffi.Mapim.MAX_BACKGROUND)
            args.n_background = len(background)
            args.background[:len(background)] = background
        args.premultiplied = int(bool(premultiplied))
        return args

    def mapim(self, index, interpolate="bilinear", extend="background", background=0, premultiplied=False):
        """vips_mapim: pel (x, y) of the result is this image resampled at the coordinate pel (x, y) of ``index`` holds
        (two bands, or one complex band); the result has the index's size.  interpolate "nearest" / "bilinear" /
        "bicubic"; extend, background and premultiplied as in pyvips."""
        if not isinstance(index, Image):
            raise TypeError("mapim: the index must be an Image")
        out = ctypes.c_void_p()
        check(lib.vips_hip_mapim(self._h, index._h, ctypes.byref(out),
                                 ctypes.byref(self.mapim_args(interpolate, extend, background, premultiplied))))
        return Image(out.value)

    # libvips/convolution: vips_fastcor / vips_spcor
    def fastcor(self, ref):
        """vips_fastcor: the sum of squared differences between ``ref`` and the window of this image at every pel (uint,
        float or double; the image is extended by copies of its edges and shifted by half the ref).  The best match is
        ``fastcor(ref).min(with_options=True)``."""
        if not isinstance(ref, Image):
            raise TypeError("fastcor: the ref must be an Image")
        return self._binary(lib.vips_hip_fastcor, ref)

    def spcor(self, ref):
        """vips_spcor: the normalised correlation coefficient of ``ref`` and the window of this image at every pel, a
        float image; 0 where the ref or the window is constant."""
        if not isinstance(ref, Image):
            raise TypeError("spcor: the ref must be an Image")
        return self._binary(lib.vips_hip_spcor, ref)

    @classmethod
    def xyz(cls, width, height):
        """vips_xyz: a two-band uint image whose pel (x, y) holds (x, y), made on the device."""
        out = ctypes.c_void_p()
        check(lib.vips_hip_xyz(ctypes.byref(out), int(width), int(height)))
        return cls(out.value)

    # vips_embed / vips_gravity / vips_flatten / vips_addalpha / vips_insert / vips_join, with pyvips' argument names
    @staticmethod
    def _background(args, background, what):
        if background is not None:
            background = [float(v) for v in np.atleast_1d(background)]
            if len(background) > _ffi.Embed.MAX_BACKGROUND:
                raise _ffi.VipsHipError("%s: background of more than %d elements" % (what, _ffi.Embed.MAX_BACKGROUND))
            args.n_background = len(background)
            args.background[:len(background)] = background
        return args

    @classmethod
    def embed_args(cls, extend=None, background=None):
        """The VipsHipEmbed of these arguments: ``extend`` None means not given (a background then selects extend
        "background", as in vips_embed)."""
        args = _ffi.Embed()
        lib.vips_hip_embed_defaults(ctypes.byref(args))
        if extend is not None:
            args.extend = _enum(EXTENDS, extend, "extend")
            args.extend_set = 1
        return cls._background(args, background, "embed")

    def embed(self, x, y, width, height, extend=None, background=None):
        """vips_embed: the image at (x, y) on a canvas of width x height; extend "black" (the default), "copy",
        "repeat", "mirror", "white" or "background"."""
        return self._unary(lib.vips_hip_embed, int(x), int(y), int(width), int(height),
                           ctypes.byref(self.embed_args(extend, background)))

    def gravity(self, direction, width, height, extend=None, background=None):
        """vips_gravity: the image placed on the canvas by a compass direction ("centre", "north", "north-east" ...)."""
        return self._unary(lib.vips_hip_gravity, _enum(COMPASS_DIRECTIONS, direction, "direction"), int(width), int(height),
                           ctypes.byref(self.embed_args(extend, background)))

    def flatten(self, background=None, max_alpha=None):
        """vips_flatten: the last band blended out against ``background`` (default 0); ``max_alpha`` defaults to the
        interpretation's (255, 65535 for 16-bit, 1 for scRGB)."""
        args = _ffi.Flatten()
        lib.vips_hip_flatten_defaults(ctypes.byref(args))
        self._background(args, background, "flatten")
        if max_alpha is not None:
            args.max_alpha_set = 1
            args.max_alpha = float(max_alpha)
        return self._unary(lib.vips_hip_flatten, ctypes.byref(args))

    def addalpha(self):
        """vips_addalpha: one more band holding the interpretation's max alpha."""
        return self._unary(lib.vips_hip_addalpha)

    @classmethod
    def _insert_args(cls, expand, background, shim=0, align="low"):
        args = _ffi.Insert()
        lib.vips_hip_insert_defaults(ctypes.byref(args))
        args.expand = int(bool(expand))
        args.shim = int(shim)
        args.align = _enum(ALIGNS, align, "align")
        return cls._background(args, background, "insert")

    def insert(self, sub, x, y, expand=False, background=None):
        """vips_insert: ``sub`` pasted onto this image at (x, y); formats and bands are matched as the reference does."""
        out = ctypes.c_void_p()
        check(lib.vips_hip_insert(self._h, sub._h, ctypes.byref(out), int(x), int(y),
                                  ctypes.byref(self._insert_args(expand, background))))
        return Image(out.value)

    def join(self, other, direction, expand=False, shim=0, background=None, align="low"):
        """vips_join: ``other`` beside ("horizontal") or below ("vertical") this image."""
        out = ctypes.c_void_p()
        check(lib.vips_hip_join(self._h, other._h, ctypes.byref(out), _enum(DIRECTIONS, direction, "direction"),
                                ctypes.byref(self._insert_args(expand, background, shim, align))))
        return Image(out.value)

    # vips_arrayjoin / vips_replicate / vips_wrap / vips_grid / vips_zoom / vips_subsample, with pyvips' argument names
    @classmethod
    def arrayjoin_args(cls, across=None, shim=0, background=None, halign="low", valign="low", hspacing=None, vspacing=None):
        """The VipsHipArrayjoin of these arguments: None means not given."""
        args = _ffi.Arrayjoin()
        lib.vips_hip_arrayjoin_defaults(ctypes.byref(args))
        for name, value in (("across", across), ("hspacing", hspacing), ("vspacing", vspacing)):
            if value is not None:
                if int(value) < 1:
                    raise _ffi.VipsHipError("arrayjoin: %s must be at least 1" % name)
                setattr(args, name, int(value))
        args.shim = int(shim)
        args.halign = _enum(ALIGNS, halign, "halign")
        args.valign = _enum(ALIGNS, valign, "valign")
        return cls._background(args, background, "arrayjoin")

    @staticmethod
    def arrayjoin(images, across=None, shim=0, background=None, halign="low", valign="low", hspacing=None, vspacing=None):
        """vips_arrayjoin: the images laid out as a grid ``across`` wide (default: one row), one launch for the whole
        sheet.  Each image sits in a box of hspacing x vspacing (default: the largest image) by halign / valign; boxes
        are ``shim`` apart; what no image covers is ``background``."""
        images = list(images)
        handles = (ctypes.c_void_p * max(1, len(images)))(*[im._h for im in images])
        out = ctypes.c_void_p()
        args = Image.arrayjoin_args(across, shim, background, halign, valign, hspacing, vspacing)
        check(lib.vips_hip_arrayjoin(handles, len(images), ctypes.byref(out), ctypes.byref(args)))
        return Image(out.value)

    def replicate(self, across, down):
        """vips_replicate: the image ``across`` times across and ``down`` times down."""
        return self._unary(lib.vips_hip_replicate, int(across), int(down))

    def wrap(self, x=None, y=None):
        """vips_wrap: the image's origin moved to (x, y), what leaves at one side comes back at the other; the defaults
        are the centre."""
        return self._unary(lib.vips_hip_wrap, int(x or 0), int(y or 0), int(x is not None), int(y is not None))

    def grid(self, tile_height, across, down):
        """vips_grid: a tall strip of across * down tiles of ``tile_height`` rows laid out as a grid."""
        return self._unary(lib.vips_hip_grid, int(tile_height), int(across), int(down))

    def zoom(self, xfac, yfac):
        """vips_zoom: every pel ``xfac`` times across and ``yfac`` times down."""
        return self._unary(lib.vips_hip_zoom, int(xfac), int(yfac))

    def subsample(self, xfac, yfac, point=False):
        """vips_subsample: every ``xfac``-th pel of every ``yfac``-th row.  ``point`` picks between two loops of the
        reference that make the same pels; it changes nothing here."""
        return self._unary(lib.vips_hip_subsample, int(xfac), int(yfac))

    # vips_linear / vips_invert / vips_abs, vips_add / vips_subtract / vips_multiply / vips_divide, vips_stats and its
    # single-number siblings, with pyvips' argument names
    @staticmethod
    def linear_args(a, b, uchar=False):
        """The VipsHipLinear of these arguments: ``a`` and ``b`` numbers or vectors of 1 or ``bands`` elements."""
        args = _ffi.Linear()
        lib.vips_hip_linear_defaults(ctypes.byref(args))
        for name, vector in (("a", a), ("b", b)):
            vector = [float(v) for v in np.atleast_1d(vector)]
            if not 1 <= len(vector) <= _ffi.Linear.MAX_VECTOR:
                raise _ffi.VipsHipError("linear: vectors of 1 to %d elements" % _ffi.Linear.MAX_VECTOR)
            setattr(args, "n_" + name, len(vector))
            getattr(args, name)[:len(vector)] = vector
        args.uchar = int(bool(uchar))
        return args

    def linear(self, a, b, uchar=False):
        """vips_linear: ``self * a + b``, float (double for a double image), or uchar with ``uchar=True``; a one-band
        image against n-element vectors makes n bands."""
        return self._unary(lib.vips_hip_linear, ctypes.byref(self.linear_args(a, b, uchar)))

    def invert(self):
        """vips_invert: the format's maximum less the value for unsigned formats, the negative otherwise."""
        return self._unary(lib.vips_hip_invert)

    def abs(self):
        """vips_abs."""
        return self._unary(lib.vips_hip_abs)

    def _binary(self, fn, other):
        out = ctypes.c_void_p()
        check(fn(self._h, other._h, ctypes.byref(out)))
        return Image(out.value)

    def add(self, other):
        """vips_add: formats, bands (one against n) and sizes are matched as the reference matches them."""
        return self._binary(lib.vips_hip_add, other)

    def subtract(self, other):
        return self._binary(lib.vips_hip_subtract, other)

    def multiply(self, other):
        return self._binary(lib.vips_hip_multiply, other)

    def divide(self, other):
        """vips_divide: 0 where ``other`` is 0."""
        return self._binary(lib.vips_hip_divide, other)

    # vips_round / vips_sign / vips_clamp, vips_minpair / vips_maxpair, vips_remainder / vips_remainder_const
    ROUND = {"rint": 0, "ceil": 1, "floor": 2}

    def round(self, round):
        """vips_round: ``"rint"``, ``"ceil"`` or ``"floor"`` in the image's own type; an integer image is a copy."""
        return self._unary(lib.vips_hip_round, _enum(self.ROUND, round, "round"))

    def rint(self):
        return self.round("rint")

    def ceil(self):
        return self.round("ceil")

    def floor(self):
        return self.round("floor")

    def sign(self):
        """vips_sign: char, 1 / 0 / -1; a NaN gives -1."""
        return self._unary(lib.vips_hip_sign)

    def clamp(self, min=0.0, max=1.0):
        """vips_clamp: the larger of ``min`` and the smaller of ``max`` and the pel, stored to the image's format."""
        return self._unary(lib.vips_hip_clamp, float(min), float(max))

    def minpair(self, other):
        """vips_minpair: the smaller of the two images' elements; a NaN loses to a number."""
        return self._binary(lib.vips_hip_minpair, other)

    def maxpair(self, other):
        return self._binary(lib.vips_hip_maxpair, other)

    def remainder(self, other):
        """vips_remainder / vips_remainder_const: ``self % other``, -1 where the divisor is 0; numbers are truncated to
        int, as the reference truncates them."""
        if isinstance(other, Image):
            return self._binary(lib.vips_hip_remainder, other)
        c = self._numbers(other)
        return self._unary(lib.vips_hip_remainder_const, c.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(c))

    __mod__ = remainder

    # vips_sum / vips_bandrank, as pyvips spells them: sum is called on the class with the whole array, bandrank on the
    # first image with the others
    @staticmethod
    def _array(images, what):
        images = list(images)
        if not images or not all(isinstance(im, Image) for im in images):
            raise TypeError("%s: need a list of images" % what)
        return (ctypes.c_void_p * len(images))(*[im._h for im in images]), len(images)

    @staticmethod
    def sum(images):
        """vips_sum: the images added up in order, in uint / int / float / double; formats, bands (one against n) and
        sizes are matched as the reference matches them."""
        handles, n = Image._array(images, "sum")
        out = ctypes.c_void_p()
        check(lib.vips_hip_sum(handles, n, ctypes.byref(out)))
        return Image(out.value)

    def bandrank(self, other, index=-1):
        """vips_bandrank of self and an image or a list of images: element by element the ``index``-th smallest of the
        images' values (-1: the median)."""
        images = [self] + (list(other) if isinstance(other, (list, tuple)) else [other])
        handles, n = Image._array(images, "bandrank")
        out = ctypes.c_void_p()
        check(lib.vips_hip_bandrank(handles, n, ctypes.byref(out), int(index)))
        return Image(out.value)

    # vips_recomb
    @staticmethod
    def recomb_matrix(m):
        """A nested list or a numpy array as recomb's matrix: a contiguous (mheight, mwidth) array of doubles."""
        a = np.ascontiguousarray(m, np.float64)
        if a.ndim == 1:
            a = a[None, :]
        if a.ndim == 3 and a.shape[2] == 1:
            a = a[:, :, 0]
        if a.ndim != 2 or a.size == 0:
            raise ValueError("recomb: need a 2D matrix")
        return np.ascontiguousarray(a)

    def recomb(self, m):
        """vips_recomb: every pel's bands against the matrix ``m`` (an ``Image`` of one band, a nested list or a numpy
        array, one row an output band): float, double for a double image."""
        if isinstance(m, Image):
            return self._unary(lib.vips_hip_recomb, m._h)
        a = self.recomb_matrix(m)
        return self._unary(lib.vips_hip_recomb_matrix, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), a.shape[1], a.shape[0])

    def stats(self):
        """vips_stats: a (bands + 1, 10) array, row 0 over all bands, columns min, max, sum, sum2, avg, sd, xmin, ymin,
        xmax, ymax."""
        out = np.empty((self.bands + 1, 10), np.float64)
        check(lib.vips_hip_stats(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return out

    def avg(self):
        out = ctypes.c_double()
        check(lib.vips_hip_avg(self._h, ctypes.byref(out)))
        return out.value

    def deviate(self):
        out = ctypes.c_double()
        check(lib.vips_hip_deviate(self._h, ctypes.byref(out)))
        return out.value

    def _extreme(self, fn, with_options):
        out, x, y = ctypes.c_double(), ctypes.c_int(), ctypes.c_int()
        check(fn(self._h, ctypes.byref(out), ctypes.byref(x), ctypes.byref(y)))
        if with_options:
            return out.value, {"x": x.value, "y": y.value}
        return out.value

    def min(self, with_options=False):
        """vips_min.  ``with_options``: also return ``{"x", "y"}``, the first pel in raster order that holds it."""
        return self._extreme(lib.vips_hip_min, with_options)

    def max(self, with_options=False):
        return self._extreme(lib.vips_hip_max, with_options)

    # libvips/arithmetic: vips_project / vips_profile / vips_getpoint / vips_find_trim
    def _pair(self, fn):
        columns, rows = ctypes.c_void_p(), ctypes.c_void_p()
        check(fn(self._h, ctypes.byref(columns), ctypes.byref(rows)))
        return Image(columns.value), Image(rows.value)

    def project(self):
        """vips_project: ``(columns, rows)``, the sums of every column (width x 1) and of every row (1 x height), band by
        band; uint, int or double, interpretation histogram."""
        return self._pair(lib.vips_hip_project)

    def profile(self):
        """vips_profile: ``(columns, rows)``, for every column the y of its first non-zero element (or the height), for
        every row the x (or the width); int, interpretation histogram."""
        return self._pair(lib.vips_hip_profile)

    def getpoint(self, x, y):
        """vips_getpoint: the pel at (x, y) as a list of ``bands`` floats."""
        out = (ctypes.c_double * self.bands)()
        check(lib.vips_hip_getpoint(self._h, int(x), int(y), out, self.bands))
        return list(out)

    @staticmethod
    def find_trim_args(threshold=10.0, background=None, line_art=False):
        """The VipsHipFindTrim of these arguments."""
        args = _ffi.FindTrim()
        lib.vips_hip_find_trim_defaults(ctypes.byref(args))
        args.threshold = float(threshold)
        args.line_art = int(bool(line_art))
        if background is not None:
            background = [float(v) for v in np.atleast_1d(background)]
            if len(background) > _ffi.FindTrim.MAX_BACKGROUND:
                raise _ffi.VipsHipError("find_trim: background of more than %d elements" % _ffi.FindTrim.MAX_BACKGROUND)
            args.n_background = len(background)
            args.background[:len(background)] = background
        return args

    def find_trim(self, threshold=10.0, background=None, line_art=False):
        """vips_find_trim: ``(left, top, width, height)`` of what differs from ``background`` (default: the
        interpretation's white) by more than ``threshold`` after a 3 x 3 median (``line_art``: without it);
        ``(width, height, 0, 0)`` of the image when nothing does.  ``page = scan.extract_area(*scan.find_trim())``."""
        box = [ctypes.c_int() for _ in range(4)]
        check(lib.vips_hip_find_trim(self._h, ctypes.byref(self.find_trim_args(threshold, background, line_art)),
                                     *[ctypes.byref(v) for v in box]))
        return tuple(v.value for v in box)

    # libvips/morphology: vips_labelregions / vips_countlines
    def labelregions(self, with_options=False):
        """vips_labelregions: a one-band int mask that numbers the 4-connected regions of bytewise equal pels from 1, in
        raster order of each region's first pel.  ``with_options``: also return ``{"segments"}``, the number of regions
        plus one, as the reference counts."""
        out, segments = ctypes.c_void_p(), ctypes.c_int()
        check(lib.vips_hip_labelregions(self._h, ctypes.byref(out), ctypes.byref(segments) if with_options else None))
        mask = Image(out.value)
        if with_options:
            return mask, {"segments": segments.value}
        return mask

    def countlines(self, direction):
        """vips_countlines: the mean number of rises (below 128, then at or above it) down the columns
        (``"horizontal"`` lines) or along the rows (``"vertical"``)."""
        out = ctypes.c_double()
        check(lib.vips_hip_countlines(self._h, _enum(DIRECTIONS, direction, "direction"), ctypes.byref(out)))
        return out.value

    # the operators, as pyvips spells them: an image on the other side is the two-image operation, a number or a list
    # of numbers vips_linear.  There is no __rtruediv__: pyvips makes `2 / image` of vips_math2 (pow), which is not on
    # the device, so that spelling raises TypeError rather than leave it
    @staticmethod
    def _numbers(other):
        return np.atleast_1d(np.asarray(other, np.float64))

    def __add__(self, other):
        return self.add(other) if isinstance(other, Image) else self.linear(1, other)

    __radd__ = __add__

    def __sub__(self, other):
        return self.subtract(other) if isinstance(other, Image) else self.linear(1, -self._numbers(other))

    def __rsub__(self, other):
        return self.linear(-1, other)

    def __mul__(self, other):
        return self.multiply(other) if isinstance(other, Image) else self.linear(other, 0)

    __rmul__ = __mul__

    def __truediv__(self, other):
        return self.divide(other) if isinstance(other, Image) else self.linear(1.0 / self._numbers(other), 0)

    def __neg__(self):
        return self.linear(-1, 0)

    # vips_relational / vips_boolean with their _const forms, vips_ifthenelse and the band operations, with pyvips'
    # argument names: an image on the other side is the two-image operation, a number or a list of numbers the _const one
    RELATIONAL = {"equal": 0, "noteq": 1, "less": 2, "lesseq": 3, "more": 4, "moreeq": 5}
    BOOLEAN = {"and": 0, "or": 1, "eor": 2, "lshift": 3, "rshift": 4}

    def _logic(self, image_fn, const_fn, table, op, other, what):
        op = _enum(table, op, what)
        if isinstance(other, Image):
            out = ctypes.c_void_p()
            check(image_fn(self._h, other._h, ctypes.byref(out), op))
            return Image(out.value)
        c = self._numbers(other)
        return self._unary(const_fn, op, c.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(c))

    def relational(self, other, relational):
        """vips_relational / vips_relational_const: uchar, 255 where the comparison holds."""
        return self._logic(lib.vips_hip_relational, lib.vips_hip_relational_const, self.RELATIONAL, relational, other, "relational")

    def more(self, other):
        return self.relational(other, "more")

    def moreeq(self, other):
        return self.relational(other, "moreeq")

    def less(self, other):
        return self.relational(other, "less")

    def lesseq(self, other):
        return self.relational(other, "lesseq")

    def equal(self, other):
        return self.relational(other, "equal")

    def noteq(self, other):
        return self.relational(other, "noteq")

    def boolean(self, other, boolean):
        """vips_boolean / vips_boolean_const: integer formats keep their format, float and double are truncated to int."""
        return self._logic(lib.vips_hip_boolean, lib.vips_hip_boolean_const, self.BOOLEAN, boolean, other, "boolean")

    def andimage(self, other):
        return self.boolean(other, "and")

    def orimage(self, other):
        return self.boolean(other, "or")

    def eorimage(self, other):
        return self.boolean(other, "eor")

    def lshift(self, other):
        return self.boolean(other, "lshift")

    def rshift(self, other):
        return self.boolean(other, "rshift")

    def _imageize(self, match, value):
        """A number or a list of numbers as pyvips makes an image of it: one pel of that many bands in ``match``'s format
        (through vips_cast) and interpretation, spread to ``match``'s size on the device (embed, extend "copy"): only the
        one pel crosses the bus."""
        c = self._numbers(value).astype(np.float64)
        pel = Image.new_from_array(c.reshape(1, 1, len(c)), match.interpretation).cast(match.format)
        return pel.embed(0, 0, match.width, match.height, extend="copy")

    def ifthenelse(self, then, else_, blend=False):
        """vips_ifthenelse: ``then`` where self is non-zero, ``else_`` elsewhere; ``blend``: self as a 0 .. 255 weight.
        ``then`` and ``else_`` may be numbers or lists of numbers: they become images in the format of the other one
        (of self, where both are numbers), as in pyvips."""
        match = then if isinstance(then, Image) else else_ if isinstance(else_, Image) else self
        then = then if isinstance(then, Image) else self._imageize(match, then)
        else_ = else_ if isinstance(else_, Image) else self._imageize(match, else_)
        out = ctypes.c_void_p()
        check(lib.vips_hip_ifthenelse(self._h, then._h, else_._h, ctypes.byref(out), int(bool(blend))))
        return Image(out.value)

    def bandjoin(self, other):
        """vips_bandjoin of self and an image or a list of images, or -- numbers -- vips_bandjoin_const."""
        if not isinstance(other, (list, tuple)):
            other = [other]
        if all(not isinstance(o, Image) for o in other):
            c = self._numbers(other)
            return self._unary(lib.vips_hip_bandjoin_const, c.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(c))
        images = [self] + [o if isinstance(o, Image) else self._imageize(self, o) for o in other]
        handles = (ctypes.c_void_p * len(images))(*[im._h for im in images])
        out = ctypes.c_void_p()
        check(lib.vips_hip_bandjoin(handles, len(images), ctypes.byref(out)))
        return Image(out.value)

    def extract_band(self, band, n=1):
        return self._unary(lib.vips_hip_extract_band, int(band), int(n))

    def bandmean(self):
        return self._unary(lib.vips_hip_bandmean)

    def bandbool(self, boolean):
        return self._unary(lib.vips_hip_bandbool, _enum(self.BOOLEAN, boolean, "boolean"))

    def bandand(self):
        return self.bandbool("and")

    def bandor(self):
        return self.bandbool("or")

    def bandeor(self):
        return self.bandbool("eor")

    # (__eq__ and __ne__ stay identity: an Image is compared and hashed as an object; equal() / noteq() are the pixels')
    def __gt__(self, other):
        return self.more(other)

    def __ge__(self, other):
        return self.moreeq(other)

    def __lt__(self, other):
        return self.less(other)

    def __le__(self, other):
        return self.lesseq(other)

    def __and__(self, other):
        return self.andimage(other)

    __rand__ = __and__

    def __or__(self, other):
        return self.orimage(other)

    __ror__ = __or__

    def __xor__(self, other):
        return self.eorimage(other)

    __rxor__ = __xor__

    def __lshift__(self, other):
        return self.lshift(other)

    def __rshift__(self, other):
        return self.rshift(other)

    def __invert__(self):
        return self.eorimage(-1)  # as pyvips

    def __getitem__(self, arg):
        """Bands, as pyvips: ``im[1]``, ``im[0:3]`` (unit steps)."""
        if isinstance(arg, slice):
            start, stop, step = arg.indices(self.bands)
            if step != 1 or stop <= start:
                raise IndexError("bands: a non-empty slice of step 1")
            return self.extract_band(start, stop - start)
        i = int(arg)
        if not -self.bands <= i < self.bands:
            raise IndexError("band index out of range")
        return self.extract_band(i % self.bands)

    def conv(self, mask, scale=1.0, offset=0.0, precision="float", layers=5, cluster=1):
        m = self._mask(mask)
        if precision == "approximate":  # conv.c:99-107
            return self.conva(m, scale, offset, layers, cluster)
        return self._unary(
            lib.vips_hip_conv,
            m.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            m.shape[1],
            m.shape[0],
            float(scale),
            float(offset),
            _enum(PRECISIONS, precision, "precision"),
        )

    def conva(self, mask, scale=1.0, offset=0.0, layers=5, cluster=1):
        """vips_conva: approximate integer convolution (conva.c:1231-1280)."""
        m = self._mask(mask)
        return self._unary(
            lib.vips_hip_conva,
            m.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            m.shape[1],
            m.shape[0],
            float(scale),
            float(offset),
            int(layers),
            int(cluster),
        )

    def convasep(self, mask, scale=1.0, offset=0.0, layers=5):
        """vips_convasep: approximate separable integer convolution (convasep.c:775-828)."""
        m = self._mask(mask).reshape(-1)
        return self._unary(
            lib.vips_hip_convasep,
            m.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            m.size,
            float(scale),
            float(offset),
            int(layers),
        )

    def convsep(self, mask, scale=1.0, offset=0.0, precision="float", layers=5):
        m = self._mask(mask).reshape(-1)
        if precision == "approximate":  # convsep.c:81-87
            return self.convasep(m, scale, offset, layers)
        return self._unary(
            lib.vips_hip_convsep,
            m.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            m.size,
            float(scale),
            float(offset),
            _enum(PRECISIONS, precision, "precision"),
        )

    def gaussblur(self, sigma, min_ampl=0.2, precision="integer"):
        return self._unary(
            lib.vips_hip_gaussblur, float(sigma), float(min_ampl), _enum(PRECISIONS, precision, "precision")
        )

    def sharpen(self, sigma=0.5, x1=2.0, y2=10.0, y3=20.0, m1=0.0, m2=3.0):
        return self._unary(
            lib.vips_hip_sharpen, float(sigma), float(x1), float(y2), float(y3), float(m1), float(m2)
        )

    def gaussblur_colourspace(self, sigma, space, min_ampl=0.2, precision="integer"):
        """vips_gaussblur() then vips_colourspace(), one kernel where the image allows it
        (vips_hip_gaussblur_colourspace); the same pixels as ``.gaussblur().colourspace()``."""
        return self._unary(lib.vips_hip_gaussblur_colourspace, float(sigma), float(min_ampl),
                           _enum(PRECISIONS, precision, "precision"), _enum(INTERPRETATIONS, space, "space"))

    def colourspace(self, space):
        return self._unary(lib.vips_hip_colourspace, _enum(INTERPRETATIONS, space, "interpretation"))

    def premultiply(self, uchar=False):
        return self._unary(lib.vips_hip_premultiply, int(bool(uchar)))

    def unpremultiply(self, uchar=False):
        return self._unary(lib.vips_hip_unpremultiply, int(bool(uchar)))

    def cast(self, format):
        return self._unary(lib.vips_hip_cast, _enum(FORMATS, format, "format"))


def resize_sharpen_batch(images, scale, kernel="lanczos3", gap=2.0, sharpen=True, sigma=0.5, x1=2.0, y2=10.0,
                         y3=20.0, m1=0.0, m2=3.0, threads=8, wait=True):
    """BASELINE config 4: ``im.resize(scale).sharpen()`` over a batch of images, ``threads`` images
    in flight on their own streams (vips_hip_resize_sharpen_batch; ``wait=False``: the queued
    form, vips_hip_resize_sharpen_batch_queue).  Returns a list of Images."""
    n = len(images)
    ins = (ctypes.c_void_p * n)(*[im._h for im in images])
    outs = (ctypes.c_void_p * n)()
    fn = lib.vips_hip_resize_sharpen_batch if wait else lib.vips_hip_resize_sharpen_batch_queue
    failed = fn(ins, n, outs, float(scale), _enum(KERNELS, kernel, "kernel"), float(gap),
                float(sigma) if sharpen else -1.0, float(x1), float(y2), float(y3), float(m1), float(m2), int(threads))
    result = [Image(h) if h else None for h in outs]
    if failed:
        check(-1)
    return result


def gaussmat(sigma, min_ampl, separable=False, precision="integer"):
    """vips_gaussmat (create/gaussmat.c:95-167): returns (mask 2D array, scale)."""
    buf = (ctypes.c_double * (10001 * 1))()
    scale = ctypes.c_double()
    # first ask for the width with a generous buffer when separable, else size^2
    n = lib.vips_hip_gaussmat(
        float(sigma), float(min_ampl), 1, _enum(PRECISIONS, precision, "precision"), buf, 10001,
        ctypes.byref(scale),
    )
    if n < 0:
        check(-1)
    if separable:
        return np.array(buf[:n], dtype=np.float64)[None, :], scale.value
    big = (ctypes.c_double * (n * n))()
    n2 = lib.vips_hip_gaussmat(
        float(sigma), float(min_ampl), 0, _enum(PRECISIONS, precision, "precision"), big, n * n,
        ctypes.byref(scale),
    )
    if n2 < 0:
        check(-1)
    return np.array(big[: n * n], dtype=np.float64).reshape(n, n), scale.value
