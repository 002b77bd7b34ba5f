"""CPU: the restated oracles (tests/cue_seeds_ref.py, cls_head_ref.py, dsrg_ref.py, irn_loss_ref.py, oracle/hsn_ref.py and the
normalisations of oracle/cnn_ref.py) against what the REFERENCE's own functions returned: the fixtures tests/golden/ref_*.npz,
written by oracle/gen_golden_ref.py from the reference's modules loaded under stubs (oracle/ref_import.py).

  fixture against oracle     always runs; needs no reference tree.  The rule per piece is gen_golden_ref.verify's: exact, except
                             cue-seed pixels in the oracle's `ambiguous` mask (equal-area ties, painted in np.argsort's
                             unspecified order; at most 10 % of a case) and the IRNet loss values, which are float64 sums of the
                             fixture's per-pair tensors held to irn_loss_ref.loss_bound.
  fixture against reference  where the reference tree is present: the generator's computation again, in memory, array by array.
  the stubs bite             touching a stub raises; a load leaves sys.modules, sys.path and sys.meta_path as they were.

Regenerate with `python oracle/gen_golden_ref.py all`."""
import json
import os
import sys

import numpy as np
import pytest

from oracle import gen_golden_ref as gen
from oracle import ref_import

needs_reference = pytest.mark.skipif(not ref_import.available(), reason="the reference tree is not on this machine")


@pytest.fixture(scope="module")
def fixtures():
    return {piece: gen.load(piece) for piece in gen.PIECES}


@pytest.mark.parametrize("piece", gen.PIECES)
def test_fixture_against_restated_oracle(fixtures, piece):
    stats = gen.verify(piece, fixtures[piece])
    print("%s: %s" % (piece, json.dumps(stats, sort_keys=True)))
    assert stats["compared"] > 0
    if piece == "cue_seeds":
        total = stats["compared"] + stats["left_out"]
        assert stats["left_out"] <= gen.AMBIGUOUS_CAP * total
        assert all(gen.ambiguous_ok(name, share) for name, share in stats["ambiguous_share"].items())
    else:
        assert stats["left_out"] == 0


@pytest.mark.parametrize("piece", gen.PIECES)
def test_fixture_inputs_are_the_seeded_inputs(fixtures, piece):
    """the committed inputs are what inputs() makes: a fixture cannot drift from the cases it names"""
    want = gen.inputs(piece)
    for k, v in want.items():
        got = fixtures[piece][k]
        assert got.dtype == np.asarray(v).dtype and np.array_equal(got, v), (piece, k)
    assert set(gen.cases_of(want)) == set(gen.cases_of(fixtures[piece]))


def test_fixtures_are_small():
    for piece in gen.PIECES:
        assert os.path.getsize(gen.fixture_path(piece)) < 512 * 1024, piece


@needs_reference
@pytest.mark.parametrize("piece", gen.PIECES)
def test_fixture_against_reference_rerun(fixtures, piece):
    d, _ = gen.compute(piece)
    committed = fixtures[piece]
    assert sorted(d) == sorted(committed)
    for k in d:
        if k == "meta":  # (library versions may move; the reference's file and lines, and the notes, may not)
            a, b = json.loads(str(d[k])), json.loads(str(committed[k]))
            a.pop("versions"), b.pop("versions")
            assert a == b
            continue
        got, want = np.asarray(d[k]), committed[k]
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), \
            (piece, k)


@needs_reference
def test_stubs_raise_on_any_use():
    util = ref_import.load("02_cues/utilities.py")
    assert "cv2" in util._wsc_stubbed and "keras" in util._wsc_stubbed and isinstance(util.cv2, ref_import.StubModule)
    with pytest.raises(RuntimeError, match="resize"):
        util.cv2.resize
    with pytest.raises(RuntimeError, match="resize"):  # through the reference's own code: resize_stack calls cv2.resize
        util.resize_stack(np.zeros((1, 1, 2, 2)), (3, 3))
    with pytest.raises(RuntimeError, match="layers"):
        util.find_final_layer(type("M", (), {"layers": [object()]})())
    hsn = ref_import.load("03c_hsn/utilities.py")
    with pytest.raises(RuntimeError, match="__call__"):  # a name imported FROM a stub raises when it is used
        hsn.model_from_json("{}")
    with pytest.raises(RuntimeError, match="unary_from_softmax"):
        hsn.unary_from_softmax.anything
    with pytest.raises(RuntimeError, match="cv2"):  # modify_by_htt with images of another size reaches cv2.resize
        hsn.modify_by_htt(np.zeros((1, 29, 4, 4)), np.zeros((1, 8, 8, 3), np.uint8), ["Background"] + ["A.W"] * 28)
    dsrg = ref_import.load("03a_sec-dsrg/DSRG.py")
    assert dsrg.CC_lab is ref_import.CCLabStandIn  # the one deliberate stand-in
    with pytest.raises(RuntimeError, match="placeholder"):
        dsrg.tf.placeholder


@needs_reference
def test_a_load_leaves_the_interpreter_as_it_was():
    loads = [("02_cues/adp_cues.py", True), ("03b_irn/net/resnet50_irn.py", "03b_irn"), ("03a_sec-dsrg/DSRG.py", None)]
    for rel, with_dir in loads:  # (the first load imports installed packages for good -- scipy, torch: they are no stand-ins)
        ref_import.load(rel, with_dir=with_dir)
    modules, path, meta, cwd = dict(sys.modules), list(sys.path), list(sys.meta_path), os.getcwd()
    mods = [ref_import.load(rel, with_dir=with_dir) for rel, with_dir in loads]
    assert sys.modules == modules and all(sys.modules[k] is modules[k] for k in modules)
    assert sys.path == path and sys.meta_path == meta and os.getcwd() == cwd
    assert not any(isinstance(m, ref_import.StubModule) for m in sys.modules.values())
    assert not any(k in sys.modules for k in ("keras", "cv2", "utilities", "net", "lib"))
    # the same file twice: two modules under two names, neither registered
    a, b = ref_import.load("02_cues/utilities.py"), ref_import.load("03c_hsn/utilities.py")
    assert a.__name__ != b.__name__ and a.__name__ not in sys.modules and hasattr(b, "dcrf_process") and not hasattr(a, "dcrf_process")
    assert mods[0].get_fg_cues.__code__.co_filename.endswith(os.path.join("02_cues", "utilities.py"))  # its own sibling


def test_missing_reference_file_is_an_error():
    with pytest.raises(FileNotFoundError):
        ref_import.load("no/such/file.py", root=os.path.dirname(os.path.abspath(__file__)))
