"""The parameter codec (_lib.flatten / _lib.unflatten and the three fields() tables) against the stored orders stated element by
element: no GPU, no library -- layouts and arrays in.

Layouts: the seg and irn layouts and the cls layouts tests/golden/train_plans.json records (of the two VGG16 stacks the entries
below PREFIX floats, a layout of its own as far as the codec is concerned), and three small ones typed in here whose channel counts
tell every axis apart: Cin = 3, Cout = 5, a 1 x 1 head with Cin != Cout, a Linear of more rows than the net has classes.
Every tensor is filled from one arange over the whole state dict, so no two elements are equal; where element (co, ci, ky, kx)
must lie is index arithmetic over np.indices, never a transpose or reshape that mirrors the implementation."""
import json
import os
import re

import numpy as np
import pytest

from wsscam import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_plans.json")
SENTINEL = np.float32(-1.0)
PREFIX = 400000


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _named(rows, with_linear):
    keys = ("name", "conv", "linear", "shape", "offset", "size") if with_linear else ("name", "conv", "shape", "offset", "size")
    return [dict(zip(keys, r), shape=tuple(r[keys.index("shape")])) for r in rows]


def _layouts():
    with open(GOLDEN) as f:
        g = json.load(f)
    out = []
    for name, v in g["seg"].items():
        out.append(("seg", "seg-" + name, {r[0]: dict(zip(("k", "Cin", "Cout", "w_off", "b_off"), r[1:])) for r in v["layout"]}))
    out.append(("seg", "seg-small", {"a": {"k": 3, "Cin": 3, "Cout": 5, "w_off": 0, "b_off": 135}, "b": {"k": 1, "Cin": 5, "Cout": 7, "w_off": 140, "b_off": 175}}))
    for name, v in g["irn"].items():
        out.append(("irn", "irn-" + name, _named(v["layout"], False)))
    out.append(("irn", "irn-small", _named([["h.0.weight", True, [5, 3, 1, 1], 0, 15], ["h.1.weight", False, [5], 15, 5], ["h.1.bias", False, [5], 20, 5],
                                            ["e.weight", True, [1, 7, 1, 1], 25, 7], ["e.bias", False, [1], 32, 1]], False)))
    for name, v in g["cls"].items():
        cut = (lambda rows: rows) if name.startswith("m7") else (lambda rows: [r for r in rows if r[-2] + r[-1] <= PREFIX])
        out.append(("cls", "cls-grad-" + name, _named(cut(v["layout"]), False)))
        out.append(("cls", "cls-param-" + name, _named(cut(v["param_layout"]), True)))
    out.append(("cls", "cls-small", _named([["r.layer1.0.weight", True, False, [5, 3, 3, 3], 0, 135], ["r.layer1.0.bias", False, False, [5], 135, 5],
                                            ["r.layer1.2.weight", True, False, [7, 5, 3, 3], 140, 315], ["r.layer1.2.bias", False, False, [7], 455, 7],
                                            ["r.classifier.0.weight", False, True, [4, 7], 462, 28], ["r.classifier.0.bias", False, False, [4], 490, 4]], True)))
    return out


LAYOUTS = _layouts()


def _fields(path, layout):
    return {"seg": _lib.SegGrad, "irn": _lib.IrnGrad, "cls": _lib.ClsGrad}[path].fields(layout)


def _tensors(path, layout, extra_rows=0):
    """-> ([(key, shape as the caller sees it, offset, tensor)], the nested / flat dict flatten takes); values 1, 2, 3, ... over
    the whole dict.  extra_rows: the classifier's tensors get that many rows more than the layout has"""
    if path == "seg":
        specs = [((n, w), (e["k"], e["k"], e["Cin"], e["Cout"]) if w == "w" else (e["Cout"],), e[w + "_off"]) for n, e in layout.items() for w in ("w", "b")]
    else:
        specs = [(e["name"], tuple(e["shape"]), e["offset"]) for e in layout]
    items, d, at = [], {}, 1
    for key, shape, off in specs:
        full = (shape[0] + extra_rows,) + shape[1:] if extra_rows and ".classifier." in str(key) else shape
        t = np.arange(at, at + int(np.prod(full)), dtype=np.float32).reshape(full)
        at += t.size
        items.append((key, shape, off, t))
        if isinstance(key, tuple):
            d.setdefault(key[0], {})[key[1]] = t
        else:
            d[key] = t
    assert at < 2 ** 24  # every value is exact in float32: no two elements are equal
    return items, d


def _positions(path, shape, off):
    """where each element of a tensor of `shape` must lie in the flat buffer, as an index array of that shape"""
    ix = np.indices(shape)
    if path == "seg" and len(shape) == 4:    # HWIO as it is: [ky][kx][ci][co]
        ky, kx, ci, co = ix
        return off + ((ky * shape[1] + kx) * shape[2] + ci) * shape[3] + co
    if path == "irn" and len(shape) == 4:    # OIHW 1 x 1 stored as [Cin][Cout]
        co, ci, ky, kx = ix
        assert shape[2:] == (1, 1)
        return off + ci * shape[0] + co
    if path == "cls" and len(shape) == 4:    # OIHW 3 x 3 stored as [3][3][Cin][Cout]
        co, ci, ky, kx = ix
        assert shape[2:] == (3, 3)
        return off + ((ky * 3 + kx) * shape[1] + ci) * shape[0] + co
    if len(shape) == 2:                      # the Linear [C][F] as it is
        return off + ix[0] * shape[1] + ix[1]
    return off + ix[0]                       # a vector


@pytest.mark.parametrize("path,name,layout", LAYOUTS, ids=[l[1] for l in LAYOUTS])
def test_every_element_lies_where_the_stored_order_says(path, name, layout):
    fields = _fields(path, layout)
    items, tensors = _tensors(path, layout)
    elems = sum(f.size for f in fields)
    assert elems == max(f.offset + f.size for f in fields) == sum(int(np.prod(s)) for _, s, _, _ in items)  # no gaps, no overlap
    want = np.full(elems, SENTINEL, np.float32)
    for key, shape, off, t in items:
        pos = _positions(path, shape, off)
        assert (want[pos] == SENTINEL).all(), key  # written once
        want[pos] = t
    assert not (want == SENTINEL).any()  # every float of the buffer is some tensor's
    flat = _lib.flatten(tensors, fields)
    assert flat.dtype == np.float32 and flat.shape == (elems,)
    assert np.array_equal(_bits(flat), _bits(want)), (name, int((_bits(flat) != _bits(want)).sum()))
    assert np.array_equal(_bits(_lib.flatten(tensors, fields, elems + 3)[:elems]), _bits(want))  # a longer buffer: the same front
    back = _lib.unflatten(flat, fields)
    for key, shape, off, t in items:
        got = back[key[0]][key[1]] if isinstance(key, tuple) else back[key]
        assert got.shape == shape and got.dtype == np.float32 and got.flags["C_CONTIGUOUS"], key
        assert np.array_equal(_bits(got), _bits(t)), key
    assert sum(len(v) if isinstance(v, dict) else 1 for v in back.values()) == len(items)


def test_classifier_rows_beyond_the_classes_are_cut():
    path, name, layout = LAYOUTS[-1]
    fields = _fields(path, layout)
    items, tensors = _tensors(path, layout, extra_rows=3)
    assert tensors["r.classifier.0.weight"].shape == (7, 7) and tensors["r.classifier.0.bias"].shape == (7,)
    flat = _lib.flatten(tensors, fields)
    for key, shape, off, t in items:
        assert np.array_equal(_bits(flat[_positions(path, shape, off)]), _bits(t[:shape[0]])), key
    back = _lib.unflatten(flat, fields)
    assert back["r.classifier.0.weight"].shape == (4, 7) and np.array_equal(back["r.classifier.0.weight"], tensors["r.classifier.0.weight"][:4])
    assert np.array_equal(back["r.classifier.0.bias"], tensors["r.classifier.0.bias"][:4])
    short = dict(tensors)
    short["r.classifier.0.weight"] = tensors["r.classifier.0.weight"][:3]  # fewer rows than classes
    with pytest.raises(ValueError, match="classifier.0.weight"):
        _lib.flatten(short, fields)
    wide = dict(tensors)
    wide["r.layer1.0.bias"] = np.zeros(8, np.float32)  # only the classifier is cut
    with pytest.raises(ValueError, match="layer1.0.bias"):
        _lib.flatten(wide, fields)


@pytest.mark.parametrize("path,name,layout", [l for l in LAYOUTS if l[1].endswith("-small")], ids=["seg", "irn", "cls"])
def test_refusals_name_the_tensor(path, name, layout):
    fields = _fields(path, layout)
    items, tensors = _tensors(path, layout)
    for key, shape, off, t in items:
        missing = {k: (dict(v) if isinstance(v, dict) else v) for k, v in tensors.items()}
        wrong = {k: (dict(v) if isinstance(v, dict) else v) for k, v in tensors.items()}
        if isinstance(key, tuple):
            del missing[key[0]][key[1]]
            wrong[key[0]][key[1]] = np.zeros(shape + (1,), np.float32)
        else:
            del missing[key]
            wrong[key] = np.zeros(shape[::-1] + (2,), np.float32)
        with pytest.raises(ValueError, match=re.escape(repr(key))):
            _lib.flatten(missing, fields)
        with pytest.raises(ValueError, match=re.escape(repr(key))):
            _lib.flatten(wrong, fields)
    if path == "seg":  # a whole layer missing
        with pytest.raises(ValueError, match="'b'"):
            _lib.flatten({"a": tensors["a"]}, fields)
