"""The seven predictors of the device JPEG Lossless encoder and its choice among them, on top of tests/jpeg_lossless_model.py:
the cost by which predictor 0 ("auto") chooses, restated, and the rasters and cases that tests/test_jpeg_lossless_predictors_host.py
and tests/test_gpu_jpeg_lossless_predictors.py share."""
import functools

import numpy as np

import jpeg_lossless_model as m

PREDICTORS = tuple(range(1, 8))
PRECISIONS = {8: np.uint8, 12: np.uint16, 16: np.uint16}
RESTARTS = (0, 1, 2, 5)
SHAPES = tuple((rows, cols) for rows in m.ROWS for cols in m.COLS)


def auto_cost(img, P, ss, restart_rows=0):
    """bits by which the device weighs selection value ss for this frame: every sample's code and extra bits under the Annex K.2
    table of its category histogram, and the HUFFVAL bytes of the DHT.  No byte stuffing and no pad bits."""
    d, _ = m.differences(img, P, ss, 0, restart_rows)
    hist = np.bincount(m.categories(d)[0].ravel(), minlength=17)
    bits, huffval = m.huffman_table(hist)
    size = {s: ln for s, (_, ln) in m.codes_of(bits, huffval).items()}
    return sum(int(hist[s]) * (size.get(s, 0) + (s if s < 16 else 0)) for s in range(17)) + 8 * len(huffval)


def auto_costs(img, P, restart_rows=0):
    return [auto_cost(img, P, ss, restart_rows) for ss in PREDICTORS]


def auto_pick(img, P, restart_rows=0):
    """the selection value of the smallest cost, the lowest among equals"""
    costs = auto_costs(img, P, restart_rows)
    return 1 + costs.index(min(costs))


def sos_predictor(f):
    """Ss of a file this project writes: one scan, and no 0xFF 0xDA before its SOS"""
    return f[f.index(b"\xff\xda") + 7]


# ---- planted rasters: what auto must answer ------------------------------------------------------------------------------

def constant(rows=16, cols=24, value=100):
    """every difference but the first is 0 under all seven: a tie of all, so 1"""
    return np.full((rows, cols), value, np.uint8)


def vertical_stripes(rows=16, cols=24):
    """x depends on the column alone: Rb is exact, and so are Ra + Rb - Rc and Rb + ((Ra - Rc) >> 1) -- 2, 4 and 6 tie and 2,
    the lowest, is the answer; Ra misses every sample"""
    f = np.random.default_rng(5).integers(0, 256, cols)
    return np.broadcast_to(f, (rows, cols)).astype(np.uint8)


def falling_plane(rows=16, cols=24):
    """x = 128 - c + r: Rc is exact, and so are Ra + Rb - Rc (a plane), Ra + ((Rb - Rc) >> 1) = Ra + (-1 >> 1) = Ra - 1 and
    (Ra + Rb) >> 1 = (2 x) >> 1 -- 3, 4, 5 and 7 tie below the other three (Ra, Rb and Rb + ((Ra - Rc) >> 1) = Rb are off by one
    everywhere), so 3"""
    rr, cc = np.mgrid[0:rows, 0:cols]
    return (128 - cc + rr).astype(np.uint8)


def planted():
    """name -> (raster, precision, the selection value auto must choose)"""
    return {"constant": (constant(), 8, 1), "vertical_stripes": (vertical_stripes(), 8, 2), "falling_plane": (falling_plane(), 8, 3)}


@functools.lru_cache(maxsize=None)
def golden_slice(name="slice0671"):
    """a real CT slice of tests/golden: 512 x 512 uint16 below 2^12"""
    import golden_inputs as gi
    return np.ascontiguousarray(gi.load_slice(name)).astype(np.uint16)


# ---- differences that leave 16 bits -----------------------------------------------------------------------------------------

def wrap_rasters(rows=6, cols=9):
    """uint16 rasters of precision 16 on which selection values 4 .. 6 predict outside 0 .. 65535 and the difference 0x8000
    (category 16) occurs"""
    rr, cc = np.mgrid[0:rows, 0:cols]
    spike = np.zeros((rows, cols), np.uint16)
    spike[rows // 2, cols // 2] = 65535
    return {
        "checkerboard": np.where((rr + cc) % 2 == 0, 0, 65535).astype(np.uint16),
        "alternating_rows": np.where(rr % 2 == 0, 0, 65535).astype(np.uint16) + np.zeros((rows, cols), np.uint16),
        "spike": spike,
    }
