"""NumPy restatement of the complex-baseband discriminator (include/gnuais_hip.h, above gnuais_batch_run_iq), operation
for operation in float32 -- the yardstick the device's iq_disc.hip is held to bit for bit.  Test code only."""
import numpy as np

_BITS = dict(A1=0x3F7FF738, A3=0xBEA91D04, A5=0x3E3876E2, A7=0xBDAE5A36, A9=0x3CAAAE5F,
             PI=0x40490FDB, HALF_PI=0x3FC90FDB, G=0x4622F983)
K = {k: np.array(v, dtype=np.uint32).view(np.float32)[()] for k, v in _BITS.items()}
DECIMALS = dict(A1="0.9998660", A3="-0.3302995", A5="0.1801410", A7="-0.0851330", A9="0.0208351")


def disc_pairs(I, Q, Ip, Qp) -> np.ndarray:
    """out for each (I, Q) after (Ip, Qp): arrays of any equal shape (int16 values) -> int16"""
    f = np.float32
    I, Q, Ip, Qp = (np.asarray(a).astype(f) for a in (I, Q, Ip, Qp))
    with np.errstate(invalid="ignore", divide="ignore"):
        re = (I * Ip) + (Q * Qp)
        im = (Q * Ip) - (I * Qp)
        ax, ay = np.abs(re), np.abs(im)
        mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
        t = np.where(mx == f(0), f(0), mn / mx).astype(f)
    s = t * t
    p = t * (K["A1"] + s * (K["A3"] + s * (K["A5"] + s * (K["A7"] + s * K["A9"]))))
    p = np.where(ay > ax, K["HALF_PI"] - p, p)
    p = np.where(re < f(0), K["PI"] - p, p)
    p = np.where(im < f(0), -p, p)
    o = np.clip(np.rint(p * K["G"]), f(-32768), f(32767))
    return o.astype(np.int16)


def discriminate(iq: np.ndarray, carry=None):
    """iq int16 [len][N][2] -> (audio int16 [len][N], new carry int16 [N][2]); carry (0, 0) when None"""
    iq = np.asarray(iq, dtype=np.int16)
    assert iq.ndim == 3 and iq.shape[2] == 2
    n = iq.shape[1]
    c = np.zeros((n, 2), dtype=np.int16) if carry is None else np.asarray(carry, dtype=np.int16)
    prev = np.concatenate([c[None], iq[:-1]], axis=0)
    out = disc_pairs(iq[..., 0], iq[..., 1], prev[..., 0], prev[..., 1])
    return out, iq[-1].copy()
