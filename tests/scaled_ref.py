"""The render at a delivery size (include/dvsg_amd.h, "Output size") restated in NumPy on tests/border_ref.py,
tests/bicubic_ref.py and tests/p010_ref.py: the per-sample float32 values of the view's filter and border at the VIRTUAL
grid, the row-major float32 average, the division and the byte or word rule.  Every float32 operation below is one NumPy
float32 operation, in the header's order, so the device's bytes and float32 bits are these, with no tolerance.  x_s, y_s
(the TPS map's normalised source coordinates of every virtual sample, [sy po, sx qo]) are INPUTS, as in those helpers.

A plane is [ph, pw, C] uint8 (RGB C = 3, NV12 luma C = 1, NV12 chroma C = 2) or, with p010=True, uint16 words."""
import numpy as np

import border_ref as B
import p010_ref as P

f32 = np.float32


def factors(source_size, out_size):
    """(sy, sx) = max(1, ceil(H / oh)), max(1, ceil(W / ow)), in integers"""
    (H, W), (oh, ow) = source_size, out_size
    return max(1, -(-H // oh)), max(1, -(-W // ow))


def virtual_values(plane, x_s, y_s, border, bicubic, chroma=False, p010=False):
    """v [sy po, sx qo, C] float32: the filter and border at every virtual sample, before any byte rule"""
    assert border in ("black", "replicate", "mirror")
    if p010:
        v, _ = (P.render_bicubic if bicubic else P.render_bilinear)(plane, x_s, y_s, border, chroma)
    else:
        v, _ = B.render(plane, x_s, y_s, border, bicubic, chroma)
    assert v.dtype == f32
    return v


def average(v, sy, sx):
    """[sy po, sx qo, C] -> [po, qo, C]: acc = v[0][0]; acc = acc + v[p][q] row-major; out = acc / (float)(sx sy)"""
    v = np.asarray(v)
    assert v.dtype == f32 and v.shape[0] % sy == 0 and v.shape[1] % sx == 0
    acc = None
    for p in range(sy):
        for q in range(sx):
            t = v[p::sy, q::sx]
            acc = t.copy() if acc is None else acc + t
            assert acc.dtype == f32
    out = acc / f32(sx * sy)
    assert out.dtype == f32
    return out


def to_samples(out, bicubic, chroma=False, p010=False):
    """the plane's output rule: bytes truncate (bilinear RGB / luma), round to nearest (bicubic) or at 128.5 (chroma); P010
    words round"""
    return P.to_word(out, chroma) if p010 else B.to_u8(out, bicubic, chroma)


def render(plane, x_s, y_s, sy, sx, border, bicubic, chroma=False, p010=False):
    """(out float32 [po, qo, C], its bytes or words) of one plane"""
    out = average(virtual_values(plane, x_s, y_s, border, bicubic, chroma, p010), sy, sx)
    return out, to_samples(out, bicubic, chroma, p010)


def coverage(plane_shape, x_s, y_s, sy, sx):
    """per output sample, how many of its sy sx virtual samples are valid (sampler A's rule on a plane of this shape)"""
    import bicubic_ref as R
    ok = R.valid(plane_shape[0], plane_shape[1], x_s, y_s).astype(np.int64)
    n = np.zeros((ok.shape[0] // sy, ok.shape[1] // sx), np.int64)
    for p in range(sy):
        for q in range(sx):
            n += ok[p::sy, q::sx]
    return n
