"""CPU: the numpy oracle of the debug-image renderer (tests/render_ref.py) on facts one can check by hand, against the host
renderer the package already ships (step/cam_to_ir_label.py), and wsscam.render.blend_table against the reference's literal
blend expressions for every pair of bytes.  All comparisons are on integers: zero differing bytes."""
import types

import numpy as np
import pytest

from tests import render_ref as ref
from wsscam import render

RATIOS = [0.75, 0.25, 0.3, 0.1]


def test_two_by_two_map_two_colours():
    colour, over = ref.render(np.array([[0, 1], [1, 0]]), [(10, 20, 30), (200, 100, 50)], (2, 2))
    assert over is None and colour.dtype == np.uint8
    assert colour.tolist() == [[[10, 20, 30], [200, 100, 50]], [[200, 100, 50], [10, 20, 30]]]


def test_overlay_of_200_under_128_at_three_quarters_is_146():
    """0.25 * 200 + 0.75 * 128 = 50 + 96 = 146"""
    img = np.full((1, 1, 3), 200, np.uint8)
    _, over = ref.render(np.array([[0]]), [(128, 128, 128)], (1, 1), img=img, overlay_r=0.75)
    assert over.tolist() == [[[146, 146, 146]]]
    assert render.blend_table([(128, 128, 128)], (0, 0, 0), 0.75)[0, :, 200].tolist() == [146, 146, 146]


@pytest.mark.parametrize("label", [2, 255, -1, 2 ** 31 - 1])
def test_unlisted_label_takes_other_rgb(label):
    lab = np.array([[0, label]], dtype=np.int64)
    colours = [(1, 2, 3), (4, 5, 6)]
    assert ref.render(lab, colours, (1, 2))[0].tolist() == [[[1, 2, 3], [0, 0, 0]]]  # the reference leaves such a pixel at zero
    assert ref.render(lab, colours, (1, 2), other_rgb=(255, 255, 255))[0].tolist() == [[[1, 2, 3], [255, 255, 255]]]


@pytest.mark.parametrize("src,mid,out", [((7, 9), (20, 20), (13, 11)), ((41, 41), (1088, 1088), (224, 224)), ((5, 3), (4, 17), (9, 2))])
def test_two_stage_index_is_resizing_twice(src, mid, out):
    """the composed index map picks the pixel that two resizes in a row pick"""
    lab = np.arange(src[0] * src[1]).reshape(src)
    twice = ref.resize_nearest(ref.resize_nearest(lab, mid), out)
    iy = ref.nearest_index(src[0], mid[0])[ref.nearest_index(mid[0], out[0])]
    ix = ref.nearest_index(src[1], mid[1])[ref.nearest_index(mid[1], out[1])]
    assert np.array_equal(lab[iy][:, ix], twice)
    assert np.array_equal(ref.render(lab % 3, [(1, 1, 1), (2, 2, 2), (3, 3, 3)], out, mid_hw=mid)[0][:, :, 0], twice % 3 + 1)


def test_nearest_index_known_values():
    """3 -> 7: inv = 3 / 7, floor(x * inv) = 0 0 0 1 1 2 2; equal sizes pass through; 7 -> 3 picks 0 2 4"""
    assert ref.nearest_index(3, 7).tolist() == [0, 0, 0, 1, 1, 2, 2]
    assert ref.nearest_index(6, 6).tolist() == list(range(6))
    assert ref.nearest_index(7, 3).tolist() == [0, 2, 4]


@pytest.mark.parametrize("overlay_r", [0.5, 0.75])
def test_parity_with_the_shipped_ir_label_renderer(tmp_path, overlay_r):
    """step/cam_to_ir_label.py's _save (the renderer the package ships today: _colour and its overlay line) on a random image and
    label map, its PNGs decoded.  That line blends in float32 (np.float32(img)), the oracle in float64 as 03c / 03a / 02_cues do:
    at these ratios, whose products with a byte are exact in both formats, the truncated bytes agree (at 0.3 they do not)."""
    from PIL import Image

    from wsscam.step import cam_to_ir_label as step

    rng = np.random.default_rng(5)
    bg, fg = [(0, 0, 0), (64, 64, 64)], [(128, 0, 0), (0, 128, 0), (11, 222, 133)]
    lab_dir, clr_dir = tmp_path / "lab", tmp_path / "clr"
    lab_dir.mkdir()
    clr_dir.mkdir()
    args = types.SimpleNamespace(class_colours={"bg": bg, "fg": fg}, overlay_r=overlay_r, ir_label_out_dir=str(lab_dir),
                                 ir_label_clr_out_dir=str(clr_dir))
    conf = rng.integers(0, 5, (37, 53)).astype(np.uint8)
    img = rng.integers(0, 256, (37, 53, 3)).astype(np.uint8)
    step._save(args, "x", conf, img)
    colour, overlay = ref.render(conf, bg + fg, conf.shape, img=img, overlay_r=overlay_r)
    assert np.array_equal(np.asarray(Image.open(str(clr_dir / "x.png"))), colour)
    assert np.array_equal(np.asarray(Image.open(str(clr_dir / "x_overlay.png"))), overlay)


@pytest.mark.parametrize("rule", ["uint8", "float256"])
@pytest.mark.parametrize("overlay_r", RATIOS)
def test_blend_table_is_the_literal_expression_for_every_byte_pair(rule, overlay_r):
    """palette entry k has the colour (k, k, k) in four tables of 64 entries (63 colours + 'other'): all 256 x 256 pairs"""
    OVERLAY_R = overlay_r
    orig_img = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (256, 256, 3))
    pred_segmask = np.broadcast_to(np.arange(256, dtype=np.float64)[:, None, None], (256, 256, 3))
    if rule == "uint8":
        want = np.uint8((1 - OVERLAY_R) * orig_img + OVERLAY_R * pred_segmask)
        want_colour = np.uint8(pred_segmask)
    else:
        want = ref.float_to_byte((1 - OVERLAY_R) * orig_img / 256.0 + OVERLAY_R * pred_segmask / 256.0)
        want_colour = ref.float_to_byte(pred_segmask / 256.0)
    for lo in range(0, 256, 64):
        grey = np.repeat(np.arange(lo, lo + 64, dtype=np.uint8)[:, None], 3, axis=1)
        table = render.blend_table(grey[:63], grey[63], overlay_r, rule)
        assert table.shape == (64, 3, 256) and table.dtype == np.uint8
        for ch in range(3):
            assert np.array_equal(table[:, ch, :], want[lo:lo + 64, :, ch])
        pal, other = render.palette_bytes(grey[:63], grey[63], rule)
        assert np.array_equal(np.concatenate([pal, other[None]]), want_colour[lo:lo + 64, 0, :])


def test_quarter_size_takes_the_width_from_the_height():
    """dsize=(shape[0] // 4, shape[1] // 4) is (width, height)"""
    assert render.quarter_size((2448, 2448, 3)) == (612, 612)
    assert render.quarter_size((16, 40)) == (10, 4)


def test_cue_label_map_refuses_overlapping_seeds_when_they_are_read_as_masks():
    from wsscam.cues import demo as cues_demo

    twice = np.array([[1, 2], [3, 3], [4, 4]], dtype=np.int64)  # classes 1 and 2 both claim pixel (3, 4)
    assert cues_demo.cue_label_map(twice, 5)[3, 4] == 1
    with pytest.raises(AssertionError):
        cues_demo.cue_label_map(twice, 5, exclusive=True)


def test_debug_image_names_are_the_file_names_without_jpg():
    """filename.replace('.jpg', ''): `<stem>.png` and `<stem>_overlay.png` are what save_pair makes of them, never `.png.png`"""
    from wsscam.cues import demo as cues_demo

    assert cues_demo.debug_image_names(["2007_000033.jpg", "a/b.jpg", "t0.png"]) == ["2007_000033", "a/b", "t0.png"]
