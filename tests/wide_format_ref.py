"""The sample formats of wideband input (GNUAIS_FMT_* in include/gnuais_hip.h) restated in NumPy: how a wide (I, Q) pair
of each format becomes the int16 pair of the channeliser's definition (tests/chan_ref.py takes it from there), and the
nearest pair of each format for a given int16 pair (what an SDR of that resolution would have written)."""
import numpy as np

FORMATS = ("cs16", "cu8", "cs8", "cf32")
VALUE = {"cs16": 0, "cu8": 1, "cs8": 2, "cf32": 3}
DTYPE = {"cs16": np.dtype("<i2"), "cu8": np.dtype("u1"), "cs8": np.dtype("i1"), "cf32": np.dtype("<f4")}
PAIR_BYTES = {"cs16": 4, "cu8": 2, "cs8": 2, "cf32": 8}


def convert(x: np.ndarray, fmt: str) -> np.ndarray:
    """components of format fmt (any shape) -> int16, the definition's table:
    cs16  v = x
    cu8   v = 256 u - 32640
    cs8   v = 256 s
    cf32  y = x * 32768 in fp32; r = rint(y), ties to even; NaN -> 0; v = clamp(r, -32768, 32767)"""
    x = np.asarray(x)
    assert x.dtype == DTYPE[fmt], (x.dtype, fmt)
    if fmt == "cs16":
        return x.astype(np.int16)
    if fmt == "cu8":
        return (x.astype(np.int32) * 256 - 32640).astype(np.int16)
    if fmt == "cs8":
        return (x.astype(np.int32) * 256).astype(np.int16)
    with np.errstate(over="ignore", invalid="ignore"):
        y = x * np.float32(32768.0)
        assert y.dtype == np.float32
        r = np.rint(y)
    r = np.where(np.isnan(r), np.float32(0.0), r)
    return np.clip(r, -32768.0, 32767.0).astype(np.int16)


def quantise(v: np.ndarray, fmt: str) -> np.ndarray:
    """int16 -> the nearest value of format fmt (round to nearest, clamped to the format's range)"""
    v = np.asarray(v, dtype=np.int16).astype(np.float64)
    if fmt == "cs16":
        return v.astype(np.int16)
    if fmt == "cu8":
        return np.clip(np.rint((v + 32640.0) / 256.0), 0, 255).astype(np.uint8)
    if fmt == "cs8":
        return np.clip(np.rint(v / 256.0), -128, 127).astype(np.int8)
    return (v / 32768.0).astype(np.float32)             # exact
