"""No GPU: which conv1 widths dvsg_locnet_create accepts.  A checkpoint's root conv [7,7,c_in,64] loads for c_in = 3 S,
1 <= S <= 16; the decision is made on the host, before any device work."""
import ctypes

import numpy as np
import pytest

CONV1 = b"stabNet/localizationNet/resnet_v1_50/conv1/weights:0"


@pytest.fixture(scope="module")
def lib():
    from coupe.dvsg_amd import _lib
    return _lib.load()


def _create_with_conv1_only(lib, c_in):
    name = (ctypes.c_char_p * 1)(CONV1)
    arr = np.zeros(max(7 * 7 * c_in * 64, 1), np.float32)
    data = (ctypes.c_void_p * 1)(arr.ctypes.data)
    nd = (ctypes.c_int * 1)(4)
    dims = (ctypes.c_int64 * 4)(7, 7, c_in, 64)
    handle = ctypes.c_void_p()
    rc = lib.dvsg_locnet_create(1, name, data, nd, dims, ctypes.byref(handle))
    assert not handle.value
    return rc, lib.dvsg_last_error_string()


@pytest.mark.parametrize("c_in", [3, 15, 21, 24, 48])
def test_a_window_of_s_frames_gets_as_far_as_the_missing_batchnorm(lib, c_in):
    """conv1 alone with c_in = 3 S: accepted as a width, then DVSG_ERR_WEIGHTS (-4) for the BatchNorm array that is not there"""
    rc, msg = _create_with_conv1_only(lib, c_in)
    assert rc == -4, (rc, msg)
    assert b"conv1/BatchNorm" in msg, msg


@pytest.mark.parametrize("c_in", [20, 51, 0])
def test_other_widths_are_unsupported_and_the_message_names_the_set(lib, c_in):
    rc, msg = _create_with_conv1_only(lib, c_in)
    assert rc == -5, (rc, msg)
    assert b"c_in = 3 S, S <= 16" in msg and (b"%d input channels" % c_in) in msg, msg
