"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/wsscam.h declares."""
import numpy as np
import pytest

from wsscam import _lib


def test_header_symbols_exported(built):
    declared = _lib.check_exports()
    assert "wsc_net_forward_cam" in declared and "wsc_crf_inference" in declared
    assert len(declared) >= 25
    assert _lib.load().wsc_version() == 100


def test_no_cpu_fallback(built):
    """Without a gfx950 device the product path must fail loudly, not fall back."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.WscError) as ei:
        _lib.Context(0)
    assert ei.value.status == _lib.WSC_ERR_NO_DEVICE


def test_mirror_modules_import(built):
    from wsscam.hsn import utilities as hsn_utilities  # noqa: F401
    from wsscam.misc import imutils, torchutils
    from wsscam.net import m7_cam, resnet50_cam, vgg16_cam  # noqa: F401
    from wsscam.step import make_cam  # noqa: F401

    assert imutils.get_strided_size((375, 500), 4) == (94, 125)
    assert imutils.get_strided_up_size((375, 500), 16) == (384, 512)
    shards = torchutils.split_dataset(list(range(10)), 4)
    assert [list(s.indices) for s in shards] == [[0, 4, 8], [1, 5, 9], [2, 6], [3, 7]]


def test_shipped_library_has_no_environment_switches(built):
    """The shipped libwsscam.so reads no WSC_* environment variable: path selectors are explicit context options
    (wsc_ctx_set_option).  Checked on the binary: no 'WSC_<NAME>' string literal is left in it."""
    import re

    from wsscam import _lib

    data = open(_lib.LIB_PATH, "rb").read()
    names = set(m.decode() for m in re.findall(rb"WSC_[A-Z][A-Z0-9_]{2,}(?=\x00)", data))
    assert not names, "environment-style names in the shipped library: %s" % sorted(names)


@pytest.mark.parametrize("keys_per_image, keys, key_off", [
    ([[3, 1], [], [0]], [3, 1, 0], [0, 2, 2, 3]),
    ([[], []], [0], [0, 0, 0]),  # no key at all: one zero, so that the array has an address to hand to C
    ([[5, 2, 7]], [5, 2, 7], [0, 3]),
    ([[]], [0], [0, 0]),
])
def test_key_table(keys_per_image, keys, key_off):
    """_lib._key_table: the ragged per-image keys as one int32 array (length >= 1) + int32 offsets."""
    k, off = _lib._key_table(keys_per_image)
    assert k.dtype == np.int32 and off.dtype == np.int32 and k.flags["C_CONTIGUOUS"] and off.flags["C_CONTIGUOUS"]
    assert k.tolist() == keys and off.tolist() == key_off
    k2, off2 = _lib._key_table(keys_per_image + [[9, 9]], len(keys_per_image))  # B: only the first B images count
    assert k2.tolist() == keys and off2.tolist() == key_off


@pytest.mark.parametrize("sizes, expect", [
    ([(3, 5), (4, 4), (1, 7)], [[3, 5], [4, 4], [1, 7]]),
    ([(321, 500)], [[321, 500]]),
    (np.array([7, 9, 2, 3], np.int64), [[7, 9], [2, 3]]),  # flat input of another dtype
])
def test_size_table(sizes, expect):
    """_lib._size_table: B (height, width) pairs as C-contiguous int32 (B, 2)."""
    t = _lib._size_table(sizes, len(expect))
    assert t.dtype == np.int32 and t.shape == (len(expect), 2) and t.flags["C_CONTIGUOUS"]
    assert t.tolist() == expect
    with pytest.raises(ValueError):
        _lib._size_table(sizes, len(expect) + 1)
