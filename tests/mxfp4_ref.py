"""CPU reference for MXFP4 expert weights (torch_dtype 6): the exact dequant

    W_eff[r, c] = e2m1(nibble[r, c]) * 2^(s[r][c // 32] - 127)

in the float [.., mats, P, H] layout of the existing reference forwards.
Element k of a row lives in byte k // 2, even k in the low nibble."""
import numpy as np

E2M1 = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], dtype=np.float32)


def dequant(w_u8, s_u8):
    """w_u8 [nE, mats, P, H/2], s_u8 [nE, mats * P * H / 32] (records s_up |
    s_dn | s_glu) -> fp32 [nE, mats, P, H]; what exceeds fp32 is infinite."""
    w_u8, s_u8 = np.asarray(w_u8), np.asarray(s_u8)
    nE, mats, P, H2 = w_u8.shape
    codes = np.stack([w_u8 & 15, w_u8 >> 4], axis=-1).reshape(nE, mats, P, 2 * H2)
    vals = np.where(codes & 8, -E2M1[codes & 7], E2M1[codes & 7])
    # records are (up, down, glu) = slots (0, 1, 2), each in flat slab order
    scale = np.exp2(s_u8.astype(np.float64) - 127.0).reshape(nE, mats, -1, 1)
    with np.errstate(over="ignore"):
        return (vals.reshape(nE, mats, -1, 32) * scale).reshape(
            nE, mats, P, 2 * H2).astype(np.float32)
