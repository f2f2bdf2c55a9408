"""The cases of tests/golden/resize_ycc_layout_parity.npz and their replay: what lanczos_ycc{,16}_{source,dest}_validate return for
drawn layout structs, and what lanczos_ycc{,16}_{source,dest}_init return and fill.  The fixture is recorded from the build of ONE
commit (tests/golden/make_resize_ycc_layout_golden.py) and replayed on every later one by tests/test_resize_ycc_layout_host.py:
the validators of the four entries are one resolver now, and this holds it to what the four separate ones answered.

A case is a row of int64: VALIDATE rows are (B, dest, in_w, in_h, out_w, out_h, has_win, x0, y0, w, h, y_row_stride,
c_row_stride, cb_offset, cr_offset, layout, sub_x, sub_y, reserved word index or -1); INIT rows are (B, dest, in_w, in_h, out_w,
out_h, has_win, x0, y0, w, h, layout, sub_x, sub_y).  B is the bytes of a sample (1: the 8-bit entries, 2: the 16-bit ones)."""
import ctypes

import numpy as np

import lanczos_hls_amd as L

SEED = 20261021
N_VALIDATE = 4000
N_INIT = 600
FILL = 0x5A          # what an init case's struct holds before the call: a field the entry leaves alone shows it
LAYOUTS = (L.YCC_PLANAR, L.YCC_NV12, L.YCC_NV21)


def _desc(B, in_w, in_h, out_w, out_h):
    return L.resize_desc(int(in_w), int(in_h), int(out_w), int(out_h), 3, bits=8 * int(B))


def _window(row):
    has_win, x0, y0, w, h = (int(v) for v in row)
    if not has_win:
        return None
    win = L.ResizeWindow()
    win.x0, win.y0, win.w, win.h = x0, y0, w, h
    return win


def _draw_frame(rng, dest):
    """sizes 1 .. 9 and, of a destination, a window inside the output as often as not: origins odd and even"""
    in_w, in_h, out_w, out_h = (int(v) for v in rng.integers(1, 10, 4))
    win = (0, 0, 0, 0, 0)
    w, h = in_w, in_h
    if dest:
        w, h = out_w, out_h
        if rng.integers(2):
            w, h = int(rng.integers(1, out_w + 1)), int(rng.integers(1, out_h + 1))
            win = (1, int(rng.integers(0, out_w - w + 1)), int(rng.integers(0, out_h - h + 1)), w, h)
    return (in_w, in_h, out_w, out_h) + win, w, h


def draw_validate(rng):
    B, dest = int(rng.integers(1, 3)), int(rng.integers(2))
    frame, w, h = _draw_frame(rng, dest)
    layout, sx, sy = int(rng.choice(LAYOUTS)), int(rng.integers(2)), int(rng.integers(2))
    nv = layout != L.YCC_PLANAR
    if nv:
        sx = 1
    cw, ch = (w + sx) >> sx, (h + sy) >> sy
    c_row = (2 if nv else 1) * B * cw
    # a legal layout with padding in words, Cb and Cr in either order
    y_rs = B * (w + int(rng.integers(0, 3)))
    c_rs = c_row + B * int(rng.integers(0, 3))
    first = h * y_rs + B * int(rng.integers(0, 3))
    second = first if nv else first + ch * c_rs + B * int(rng.integers(0, 3))
    cb, cr = (first, second) if rng.integers(2) else (second, first)
    res = -1
    m = int(rng.integers(0, 24))   # 0 .. 9: as drawn; the rest moves one thing to, below or above its bound
    step = int(rng.choice((-B, -1, 0, 1, B)))
    if m == 10:
        y_rs = B * w + step
    elif m == 11:
        c_rs = c_row + step
    elif m == 12:   # the first chroma plane against the end of the luma plane
        if cb <= cr:
            cb = h * y_rs + step
            cr = cb if nv else cr
        else:
            cr = h * y_rs + step
    elif m == 13 and not nv:   # Cb over Cr: the second plane against the end of the first
        if cb <= cr:
            cr = cb + ch * c_rs + step
        else:
            cb = cr + ch * c_rs + step
    elif m == 14:
        res = int(rng.integers(0, 5))
    elif m == 15:
        layout = int(rng.choice((-1, 3, 7)))
    elif m == 16:
        sx, sy = ((2, sy), (-1, sy), (sx, 2), (sx, -1), (0, sy))[int(rng.integers(5))]   # (NV12 with sub_x 0 among them)
    elif m == 17 and nv:
        cr = cb + int(rng.choice((-B, 1, B)))
    elif m == 18:
        cb, cr = ((-1, cr), (cb, -B), (cb + (1 << 56), cr), (cb, (1 << 56) + 2))[int(rng.integers(4))]
        cr = cb if nv and rng.integers(2) else cr
    elif m == 19:
        y_rs, c_rs = (((1 << 40) + 2, c_rs), (y_rs, (1 << 40) + 2), (1 << 40, c_rs))[int(rng.integers(3))]
    elif m == 20:   # odd by one: legal for bytes, never for words
        k = int(rng.integers(4))
        y_rs, c_rs, cb, cr = y_rs + (k == 0), c_rs + (k == 1), cb + (k == 2), cr + (k == 3)
        cr = cb if nv and k == 2 else cr
    elif m == 21:   # everything one sample further: still legal
        y_rs, c_rs = y_rs + B, c_rs + B
        lo, hi = h * y_rs, h * y_rs + ch * c_rs + B
        cb, cr = ((lo, lo) if nv else (lo, hi)) if cb <= cr else (hi, lo)
    elif m == 22 and dest and frame[4]:   # the window's origin odd in x, in y, or even in both
        k = int(rng.integers(3))
        x0 = min(frame[5] | 1, frame[2] - w) if k == 0 else frame[5] & ~1 if k == 2 else frame[5]
        y0 = min(frame[6] | 1, frame[3] - h) if k == 1 else frame[6] & ~1 if k == 2 else frame[6]
        frame = frame[:5] + (x0, y0) + frame[7:]
    return (B, dest) + frame + (y_rs, c_rs, cb, cr, layout, sx, sy, res)


def draw_init(rng):
    B, dest = int(rng.integers(1, 3)), int(rng.integers(2))
    frame, _, _ = _draw_frame(rng, dest)
    layout = int(rng.choice(LAYOUTS + (3, -1))) if rng.integers(8) == 0 else int(rng.choice(LAYOUTS))
    sx, sy = (int(rng.choice((0, 1, 0, 1, 2, -1))) for _ in range(2))
    if layout != L.YCC_PLANAR and rng.integers(4):
        sx = 1
    return (B, dest) + frame + (layout, sx, sy)


def draw():
    rng = np.random.default_rng(SEED)
    validate = np.array([draw_validate(rng) for _ in range(N_VALIDATE)], dtype=np.int64)
    init = np.array([draw_init(rng) for _ in range(N_INIT)], dtype=np.int64)
    return validate, init


def _entry(lib, B, dest, what):
    return getattr(lib, "lanczos_ycc%s_%s_%s" % ("16" if B == 2 else "", "dest" if dest else "source", what))


def _ref(x):
    return ctypes.byref(x) if x is not None else None


def replay_validate(lib, cases):
    """the return code of every VALIDATE row"""
    codes = np.zeros(len(cases), np.int32)
    for i, row in enumerate(cases):
        B, dest = int(row[0]), int(row[1])
        d, win = _desc(B, *row[2:6]), _window(row[6:11])
        s = L.YccDest() if dest else L.YccSource()
        s.y_row_stride, s.c_row_stride, s.cb_offset, s.cr_offset = (int(v) for v in row[11:15])
        s.layout, s.sub_x, s.sub_y = (int(v) for v in row[15:18])
        if row[18] >= 0:
            s.reserved[int(row[18])] = 1
        fn = _entry(lib, B, dest, "validate")
        codes[i] = fn(ctypes.byref(d), _ref(win), ctypes.byref(s)) if dest else fn(ctypes.byref(d), ctypes.byref(s))
    return codes


def replay_init(lib, cases):
    """the return code of every INIT row and the 64 bytes its struct holds behind the call"""
    codes = np.zeros(len(cases), np.int32)
    filled = np.zeros((len(cases), ctypes.sizeof(L.YccSource)), np.uint8)
    for i, row in enumerate(cases):
        B, dest = int(row[0]), int(row[1])
        d, win = _desc(B, *row[2:6]), _window(row[6:11])
        s = L.YccDest() if dest else L.YccSource()
        ctypes.memset(ctypes.byref(s), FILL, ctypes.sizeof(s))
        fn = _entry(lib, B, dest, "init")
        args = (ctypes.byref(s), ctypes.byref(d)) + ((_ref(win),) if dest else ()) + tuple(int(v) for v in row[11:14])
        codes[i] = fn(*args)
        filled[i] = np.frombuffer(bytes(s), np.uint8)
    return codes, filled
