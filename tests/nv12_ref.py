"""NumPy restatement of the NV12 -> RGB conversion of include/dvsg_amd.h ("NV12 frames") and seeded NV12 batches with a
given pitch and UV offset.  int32 arithmetic with the header's table; no product imports."""
import numpy as np

BT601, BT709 = 0, 1
# matrix -> (CY, CVR, CVG, CUG, CUB), and the decimals they are int(round(c * 2**20)) of
COEF = {BT601: (1220542, 1673527, -852492, -409993, 2116026),
        BT709: (1220945, 1879825, -558796, -223608, 2215014)}
DECIMALS = {BT601: (1.164, 1.596, -0.813, -0.391, 2.018),
            BT709: (1.164384, 1.792741, -0.532909, -0.213249, 2.112402)}
SHIFT = 20


def sums(Y, U, V, matrix):
    """The three int32 sums before the shift (R, G, B), computed in int64 so that an overflow would show."""
    cy, cvr, cvg, cug, cub = COEF[matrix]
    y = np.maximum(0, np.asarray(Y, np.int64) - 16) * cy
    u, v = np.asarray(U, np.int64) - 128, np.asarray(V, np.int64) - 128
    h = 1 << (SHIFT - 1)
    return y + cvr * v + h, y + cvg * v + cug * u + h, y + cub * u + h


def yuv_to_rgb(Y, U, V, matrix):
    """uint8 [..., 3] (R, G, B) of broadcastable byte arrays Y, U, V."""
    cy, cvr, cvg, cug, cub = COEF[matrix]
    y = np.maximum(0, np.asarray(Y, np.int32) - 16) * np.int32(cy)
    u, v = np.asarray(U, np.int32) - 128, np.asarray(V, np.int32) - 128
    h = np.int32(1 << (SHIFT - 1))
    r = (y + np.int32(cvr) * v + h) >> SHIFT           # >> on a signed NumPy integer is arithmetic
    g = (y + np.int32(cvg) * v + np.int32(cug) * u + h) >> SHIFT
    b = (y + np.int32(cub) * u + h) >> SHIFT
    return np.clip(np.stack(np.broadcast_arrays(r, g, b), axis=-1), 0, 255).astype(np.uint8)


def nv12_to_rgb(y, uv, matrix, flip=0):
    """y [..., H, W], uv [..., H/2, W] (U0 V0 U1 V1 ...) -> [..., H, W, 3]; chroma of pixel (i, j) is sample (i/2, j/2)."""
    U = np.repeat(np.repeat(uv[..., 0::2], 2, axis=-2), 2, axis=-1)
    V = np.repeat(np.repeat(uv[..., 1::2], 2, axis=-2), 2, axis=-1)
    rgb = yuv_to_rgb(y, U, V, matrix)
    return np.ascontiguousarray(rgb[..., ::-1]) if flip else rgb


class Batch(object):
    """n NV12 frames of H x W in one seeded uint8 buffer [n, rows, pitch]: Y in rows [0, H), UV in rows
    [uv_row, uv_row + H/2) (uv_row >= H: a decoder's aligned luma height), every other byte seeded padding."""

    def __init__(self, seed, n, H, W, pitch=None, uv_row=None, fill=None):
        self.n, self.H, self.W = n, H, W
        self.pitch = W if pitch is None else pitch
        self.uv_row = H if uv_row is None else uv_row
        assert H % 2 == 0 and W % 2 == 0 and self.pitch >= W and self.uv_row >= H
        self.rows = self.uv_row + H // 2
        if fill is None:
            self.buf = np.random.default_rng(seed).integers(0, 256, (n, self.rows, self.pitch), dtype=np.uint8)
        else:
            self.buf = np.full((n, self.rows, self.pitch), fill, dtype=np.uint8)

    @property
    def frame_stride(self):
        return self.rows * self.pitch

    @property
    def uv_offset(self):
        return self.uv_row * self.pitch

    def planes(self, buf=None):
        """(y [n,H,W], uv [n,H/2,W]) views of `buf` (default: this batch's bytes)."""
        buf = self.buf if buf is None else buf
        return buf[:, :self.H, :self.W], buf[:, self.uv_row:self.uv_row + self.H // 2, :self.W]

    def outside(self, buf=None):
        """The bytes of `buf` that belong to neither plane."""
        buf = self.buf if buf is None else buf
        m = np.ones(buf.shape[1:], dtype=bool)
        m[:self.H, :self.W] = False
        m[self.uv_row:self.uv_row + self.H // 2, :self.W] = False
        return buf[:, m]


def smooth_batch(seed, n, H, W):
    """A packed batch [n, 3H/2, W] with smooth luma and chroma (a frame a model can stabilise)."""
    import inputs
    b = Batch(seed, n, H, W)
    f = 8 if H * W < 1 << 20 else 32
    y = inputs.smooth_frames(seed, n, H, W, C=1, factor=f)[..., 0]
    c = inputs.smooth_frames(seed + 1, n, H // 2, W // 2, C=2, factor=f)
    b.buf[:, :H] = (16 + y * 219).astype(np.uint8)
    b.buf[:, H:] = (16 + c * 224).astype(np.uint8).reshape(n, H // 2, W)
    return b
