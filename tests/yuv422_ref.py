"""4:2:2 frames (include/dvsg_amd.h, "Chroma sampling") in NumPy, no product imports: seeded NV16 / P210 batches with an
H-row UV plane, the NV12 surface the network is DEFINED to see (the Y plane and the even chroma rows; for words their high
bytes), and the index formulas of the four planar <-> semi-planar repacks.

Per-plane VALUES are not restated here: the chroma plane of a 4:2:2 frame is an image of (H, W / 2) with C = 2, and
tests/border_ref.py, tests/bicubic_ref.py, tests/p010_ref.py and tests/scaled_ref.py are already per plane.  `render_chroma`
and `render_chroma_scaled` only pick the one that belongs to the sample type."""
import numpy as np

import border_ref as B
import p010_ref as P
import scaled_ref as S


class Batch422(object):
    """n 4:2:2 frames of H x W samples in one uint8 buffer [n, rows, pitch]: Y in rows [0, H), interleaved UV in rows
    [uv_row, uv_row + H) (uv_row >= H: any row offset), `tail` rows behind them, `pitch` bytes per row (>= W bytes, words:
    even and >= 2 W).  words: P210, 16-bit little-endian words with the sample in the high 10 bits and `low` or-ed into the
    low 6; else NV16 bytes.  fill None: seeded samples with the extremes in both planes and seeded bytes everywhere else; a
    byte value: every byte that (a poisoned output)."""

    def __init__(self, seed, n, H, W, words=False, pitch=None, uv_row=None, tail=0, low=0, fill=None):
        self.n, self.H, self.W, self.is_words = n, H, W, bool(words)
        self.bps = 2 if words else 1
        self.pitch = self.bps * W if pitch is None else pitch
        self.uv_row = H if uv_row is None else uv_row
        assert H % 2 == 0 and W % 2 == 0 and self.pitch >= self.bps * W and self.pitch % self.bps == 0 and self.uv_row >= H
        self.rows = self.uv_row + H + tail
        if fill is not None:
            self.buf = np.full((n, self.rows, self.pitch), fill, dtype=np.uint8)
            return
        rng = np.random.default_rng(seed)
        self.buf = rng.integers(0, 256, (n, self.rows, self.pitch), dtype=np.uint8)
        top = 1023 if words else 255
        for lo in (0, self.uv_row):
            s = rng.integers(0, top + 1, (n, H, W), dtype=np.uint16)
            s[:, 0, 0], s[:, 0, 1], s[:, -1, -2], s[:, -1, -1] = 0, top, top, 0
            if words:
                self.buf[:, lo:lo + H, :2 * W] = ((s << 6) | np.uint16(low)).astype("<u2").view(np.uint8)
            else:
                self.buf[:, lo:lo + H, :W] = s.astype(np.uint8)

    @property
    def frame_stride(self):
        return self.rows * self.pitch

    @property
    def uv_offset(self):
        return self.uv_row * self.pitch

    def planes(self, buf=None):
        """(luma [n, H, W, 1], chroma [n, H, W / 2, 2]) copies of the two planes of `buf`: uint8, or uint16 words"""
        buf = self.buf if buf is None else buf
        H, W, n, used = self.H, self.W, self.n, self.bps * self.W
        y = np.ascontiguousarray(buf[:, :H, :used])
        uv = np.ascontiguousarray(buf[:, self.uv_row:self.uv_row + H, :used])
        if self.is_words:
            y, uv = y.view("<u2"), uv.view("<u2")
        return y.reshape(n, H, W, 1), uv.reshape(n, H, W // 2, 2)

    def outside(self, buf=None):
        """The bytes of `buf` that belong to neither plane: beyond the used bytes of a row, between the planes, behind them."""
        buf = self.buf if buf is None else buf
        m = np.ones(buf.shape[1:], dtype=bool)
        m[:self.H, :self.bps * self.W] = False
        m[self.uv_row:self.uv_row + self.H, :self.bps * self.W] = False
        return buf[:, m]


def even_rows_surface(frames, words=False):
    """The NV12 surface the network sees of packed 4:2:2 frames [..., 2 H, bps W] uint8 -> [..., 3 H / 2, W] uint8: the Y
    plane and the EVEN chroma rows; of P210 words the high byte (word >> 8) of each."""
    f = np.asarray(frames)
    assert f.dtype == np.uint8 and f.shape[-2] % 4 == 0
    H = f.shape[-2] // 2
    if words:
        f = f[..., 1::2]   # little-endian: the high byte is the second
    return np.concatenate([f[..., :H, :], f[..., H::2, :]], axis=-2)


# ---- the four repacks as index formulas on one frame's flat samples -------------------------------------------------------
def _semi_from_planar_index(H, W):
    """idx with semi.flat[e] = planar.flat[idx[e]]: Y as it is; UV sample (r, 2 c + k) is sample (r, c) of chroma plane k,
    which lies at H W + k (H W / 2) + r (W / 2) + c"""
    idx = np.arange(2 * H * W)
    r, c, k = np.meshgrid(np.arange(H), np.arange(W // 2), np.arange(2), indexing="ij")
    idx[H * W + r * W + 2 * c + k] = H * W + k * (H * W // 2) + r * (W // 2) + c
    return idx


def _planar_from_semi_index(H, W):
    """idx with planar.flat[e] = semi.flat[idx[e]]: plane k's sample (r, c) is UV sample (r, 2 c + k)"""
    idx = np.arange(2 * H * W)
    r, c, k = np.meshgrid(np.arange(H), np.arange(W // 2), np.arange(2), indexing="ij")
    idx[H * W + k * (H * W // 2) + r * (W // 2) + c] = H * W + r * W + 2 * c + k
    return idx


def i422_to_nv16(frame):
    """[2 H, W] uint8: Y, U plane, V plane -> Y, interleaved U V"""
    R, W = frame.shape
    return frame.reshape(-1)[_semi_from_planar_index(R // 2, W)].reshape(R, W)


def nv16_to_i422(frame):
    R, W = frame.shape
    return frame.reshape(-1)[_planar_from_semi_index(R // 2, W)].reshape(R, W)


def i422p10_to_p210(frame):
    """[2 H, 2 W] uint8, words with the value in the low 10 bits -> P210: word_out = (word_in << 6) mod 2^16"""
    R, W = frame.shape[0], frame.shape[1] // 2
    w = np.ascontiguousarray(frame).view("<u2").reshape(-1)[_semi_from_planar_index(R // 2, W)]
    return ((w.astype(np.uint32) << 6) & 0xFFFF).astype("<u2").view(np.uint8).reshape(R, 2 * W)


def p210_to_i422p10(frame):
    """the inverse: word_out = word_in >> 6, unsigned"""
    R, W = frame.shape[0], frame.shape[1] // 2
    w = np.ascontiguousarray(frame).view("<u2").reshape(-1)[_planar_from_semi_index(R // 2, W)]
    return (w >> 6).astype("<u2").view(np.uint8).reshape(R, 2 * W)


# ---- per-plane values: the existing references on the (H, W / 2) plane ----------------------------------------------------
def render_chroma(plane, x_s, y_s, border, bicubic, words=False):
    """(samples [H, W / 2, 2] uint8 or uint16 words, written bool [H, W / 2]) of the chroma plane of one frame at its own
    size under `border`: border_ref.render + to_u8 for bytes, p010_ref's for words"""
    if words:
        v, written = (P.render_bicubic if bicubic else P.render_bilinear)(plane, x_s, y_s, border, True)
        return P.to_word(v, True), written
    v, written = B.render(plane, x_s, y_s, border, bicubic, True)
    return B.to_u8(v, bicubic, True), written


def render_chroma_scaled(plane, x_s, y_s, sy, sx, border, bicubic, words=False):
    """samples [oh, ow / 2, 2] of the chroma plane at a delivery size: scaled_ref.render on the (H, W / 2) plane with x_s, y_s
    of the virtual grid (sy oh, sx ow / 2)"""
    return S.render(plane, x_s, y_s, sy, sx, border, bicubic, True, words)[1]
