"""A numpy model of vips_arrayjoin (conversion/arrayjoin.c) and its siblings, shared by tests/test_cells_host.py and
tests/test_cells_gpu.py, which pin it to the compiled reference through its command line; the reference's command line
itself (an array of images as one quoted argument)."""
import ctypes
import os
import subprocess

import numpy as np

from tests import helpers

VIPS = os.path.join(helpers.ROOT, "oracle", "_ref", "bin", "vips")
ALIGNS = ("low", "centre", "high")


def trunc_half(v):
    """C's int division by 2: toward zero."""
    return int(v / 2)


def plan(sizes, across=None, shim=0, halign="low", valign="low", hspacing=None, vspacing=None):
    """arrayjoin.c:231-345 for images of sizes [(w, h) ...] -> (width, height, across, rects [(l, t, w, h)], offsets
    [(x, y)]): where each image's rect lies on the output and where the image's pel (0, 0) lies in its rect."""
    n = len(sizes)
    hs = hspacing or max(w for w, _ in sizes)
    vs = vspacing or max(h for _, h in sizes)
    across = across or n
    down = -(-n // across)
    width, height = hs * across + shim * (across - 1), vs * down + shim * (down - 1)
    rects, offsets = [], []
    for i, (w, h) in enumerate(sizes):
        x, y = i % across, i // across
        rect = [x * (hs + shim), y * (vs + shim), hs + (shim if x != across - 1 else 0), vs + (shim if y != down - 1 else 0)]
        if i == n - 1:
            rect[2] = width - rect[0]
        rects.append(tuple(rect))
        offsets.append(({"low": 0, "centre": trunc_half(hs - w), "high": hs - w}[halign],
                        {"low": 0, "centre": trunc_half(vs - h), "high": vs - h}[valign]))
    return width, height, across, rects, offsets


def alike(images, n_background=1):
    """vips__formatalike_vec and vips__bandalike_vec for the promotions numpy makes as vips_cast does (a wider integer,
    float, double): the images in the common format and band count."""
    dtype = np.result_type(*[im.dtype for im in images])
    bands = max([n_background] + [im.shape[2] for im in images])
    out = []
    for im in images:
        im = im.astype(dtype)
        if im.shape[2] != bands:
            assert im.shape[2] == 1
            im = np.repeat(im, bands, axis=2)
        out.append(np.ascontiguousarray(im))
    return out


def arrayjoin(images, ink, **kw):
    """images: (h, w, b) arrays of one dtype and band count; ink: the background's pel (b elements of that dtype).
    Every rect is a vips_embed of its image at the align offset, the image cropped where it sticks out."""
    width, height, _, rects, offsets = plan([(im.shape[1], im.shape[0]) for im in images], **kw)
    out = np.empty((height, width, images[0].shape[2]), images[0].dtype)
    out[:] = ink
    for im, (l, t, w, h), (x, y) in zip(images, rects, offsets):
        cell = np.empty((h, w, im.shape[2]), im.dtype)
        cell[:] = ink
        X, Y = np.arange(w) - x, np.arange(h) - y
        xin, yin = (X >= 0) & (X < im.shape[1]), (Y >= 0) & (Y < im.shape[0])
        if xin.any() and yin.any():
            cell[np.ix_(yin, xin)] = im[Y[yin]][:, X[xin]]
        out[t:t + h, l:l + w] = cell
    return out


def replicate(src, across, down, x0=0, y0=0, width=None, height=None):
    """vips_replicate, or the window (x0, y0, width, height) of it: vips_wrap."""
    h, w = src.shape[:2]
    X = (np.arange(width if width is not None else w * across) + x0) % w
    Y = (np.arange(height if height is not None else h * down) + y0) % h
    return np.ascontiguousarray(src[Y][:, X])


def wrap_origin(size, v):
    """wrap.c:86-91, with C's remainder (the sign of the dividend)."""
    return int(np.fmod(-v, size)) if v < 0 else size - int(np.fmod(v, size))


def grid(src, tile_height, across, down):
    """vips_grid: tile i of the strip goes to (i % across, i // across)."""
    rows = []
    for ty in range(down):
        tiles = [src[(ty * across + tx) * tile_height:(ty * across + tx + 1) * tile_height] for tx in range(across)]
        rows.append(np.concatenate(tiles, axis=1))
    return np.ascontiguousarray(np.concatenate(rows, axis=0))


def ref_arrayjoin(tmp_path, images, options=()):
    """-> (array, interpretation) of `vips arrayjoin "in0.v in1.v ..." out.v [options]`; images: [(array, interpretation)];
    RuntimeError with the reference's words."""
    paths = []
    for i, (array, interp) in enumerate(images):
        paths.append(str(tmp_path / ("in%d.v" % i)))
        helpers.write_v(paths[-1], array, interp)
    out = str(tmp_path / "out.v")
    cmd = [VIPS, "arrayjoin", " ".join(paths), out] + [str(o) for o in options]
    r = subprocess.run(cmd, env=helpers.ref_cli_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr.strip() or "vips arrayjoin failed")
    return helpers.read_v(out)


def cli_options(across=None, shim=0, background=None, halign="low", valign="low", hspacing=None, vspacing=None):
    options = []
    for name, value in (("across", across), ("hspacing", hspacing), ("vspacing", vspacing)):
        if value is not None:
            options += ["--" + name, value]
    if shim:
        options += ["--shim", shim]
    if background is not None:
        options += ["--background", " ".join(repr(float(v)) for v in np.atleast_1d(background))]
    return options + ["--halign", halign, "--valign", valign]


class _Vips(object):
    lib = None


def _vips():
    """The reference's libvips.so (what oracle/_ref/lib/libref_shim.so is linked against), through ctypes."""
    if _Vips.lib is None:
        helpers.Ref.lib()  # vips_init
        v = ctypes.CDLL(os.path.join(helpers.REF_LIBDIR, "libvips.so"))
        for name in ("vips_image_new_from_memory", "vips_operation_new", "vips_image_write_to_memory"):
            getattr(v, name).restype = ctypes.c_void_p
        v.vips_image_new_from_memory.argtypes = [ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_int] * 4
        v.vips_operation_new.argtypes = [ctypes.c_char_p]
        v.vips_object_set_from_string.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
        v.vips_cache_operation_buildp.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        v.vips_image_write_to_memory.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
        v.vips_error_buffer.restype = ctypes.c_char_p
        for name in ("vips_image_get_width", "vips_image_get_height", "vips_image_get_bands", "vips_image_get_format",
                     "vips_image_get_interpretation", "g_object_unref", "vips_object_unref_outputs", "g_free"):
            getattr(v, name).argtypes = [ctypes.c_void_p]
        _Vips.lib = v
    return _Vips.lib


def ref_input(nick, array, args="", interpretation=0):
    """helpers.Ref.run_interp for the operations that name their image argument "input" (vips_zoom, vips_subsample and
    the module's classes over them): the public calls oracle/ref_shim.c makes, with that name.  -> (array,
    interpretation); RuntimeError with the reference's words."""
    v = _vips()
    a = np.ascontiguousarray(array)
    h, w, b = a.shape
    held = []

    def fail():
        message = v.vips_error_buffer().decode()
        v.vips_error_clear()
        for p in held:
            v.g_object_unref(p)
        raise RuntimeError("%s: %s" % (nick, message))

    x = v.vips_image_new_from_memory(a.ctypes.data, a.nbytes, w, h, b, helpers.DTYPE_FORMATS[a.dtype])
    if not x:
        fail()
    held.append(x)
    if interpretation > 0:
        y = ctypes.c_void_p()
        if v.vips_copy(ctypes.c_void_p(x), ctypes.byref(y), b"interpretation", ctypes.c_int(interpretation), None):
            fail()
        held.append(y.value)
        x = y.value
    op = ctypes.c_void_p(v.vips_operation_new(nick.encode()))
    if not op:
        fail()
    v.g_object_set(op, b"input", ctypes.c_void_p(x), None)
    if (args and v.vips_object_set_from_string(op, args.encode())) or v.vips_cache_operation_buildp(ctypes.byref(op)):
        held.append(op.value)
        fail()
    out = ctypes.c_void_p()
    v.g_object_get(op, b"out", ctypes.byref(out), None)
    held += [op.value, out.value]
    size = ctypes.c_size_t()
    data = v.vips_image_write_to_memory(out, ctypes.byref(size))
    if not data:
        v.vips_object_unref_outputs(op)
        fail()
    dtype = np.dtype(helpers.FORMAT_DTYPES[v.vips_image_get_format(out)])
    shape = (v.vips_image_get_height(out), v.vips_image_get_width(out), v.vips_image_get_bands(out))
    result = np.frombuffer((ctypes.c_char * size.value).from_address(data), dtype=dtype).reshape(shape).copy()
    interp = v.vips_image_get_interpretation(out)
    v.g_free(data)
    v.vips_object_unref_outputs(op)
    for p in held:
        v.g_object_unref(p)
    return result, interp
