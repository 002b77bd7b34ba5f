"""numpy restatement of the SEC / DSRG batch inputs (03a_sec-dsrg/model.py:229-270, 318-342, 698-714), independent of the package's
host twins (wsscam.secdsrg.SegBatcher.*_host, shuffled_ids): plain loops where the package indexes arrays.

  dense_cues       cues[cues_i[1], cues_i[2], cues_i[0]] = 1.0 per sample (get_data, :243-246)
  labels           label[listed] = 1.0; label[0] = 1.0 (:240-242)
  nearest_index    TF 1.x resize_nearest_neighbor(align_corners=False): scale = float32(in) / float32(out),
                   src = min((int)floor(float32(dst) * scale), in - 1) -- float32, one rounding per operation
  nearest_index_exact   the same rule in exact integer arithmetic, min(floor(dst * in / out), in - 1): what float32 departs from
  gt_index         nearest resize, then eval_miou's class test: channel 0's value (:701) or the colour table (:709-714)
  shuffle_order    dataset.repeat(-1).shuffle(n) (:278-279) given the list of slot draws"""
import numpy as np


def dense_cues(cue_lists, s, C):
    out = np.zeros((len(cue_lists), s, s, C), np.float32)
    for b, triples in enumerate(cue_lists):
        t = np.asarray(triples).reshape(3, -1)
        for k in range(t.shape[1]):
            cls, row, col = (int(v) for v in t[:, k])
            assert 0 <= cls < C and 0 <= row < s and 0 <= col < s
            out[b, row, col, cls] = 1.0
    return out


def labels(label_lists, C):
    out = np.zeros((len(label_lists), C), np.float32)
    for b, listed in enumerate(label_lists):
        for c in np.asarray(listed).reshape(-1):
            out[b, int(c)] = 1.0
        out[b, 0] = 1.0
    return out


def nearest_index(n_in, n_out):
    scale = np.float32(np.float32(n_in) / np.float32(n_out))
    idx = []
    for d in range(n_out):
        f = np.float32(np.float32(d) * scale)
        idx.append(min(int(np.floor(f)), n_in - 1))
    return np.array(idx, np.int64)


def nearest_index_exact(n_in, n_out):
    return np.array([min((d * n_in) // n_out, n_in - 1) for d in range(n_out)], np.int64)


def class_index(pixels, n_class, colours=None):
    """pixels (..., channels) uint8 -> uint8 class index in [0, n_class]"""
    px = np.asarray(pixels)
    flat = px.reshape(-1, px.shape[-1])
    out = np.full(len(flat), n_class, np.uint8)
    for i, p in enumerate(flat):
        if colours is None:
            if int(p[0]) < n_class:
                out[i] = int(p[0])
        else:
            for k in range(n_class):
                if tuple(int(v) for v in p[:3]) == tuple(int(v) for v in colours[k]):
                    out[i] = k
                    break
    return out.reshape(px.shape[:-1])


def gt_index(gt, n_class, out_hw, colours=None):
    g = np.asarray(gt)
    if g.ndim == 2:
        g = g[:, :, None]
    ys, xs = nearest_index(g.shape[0], out_hw[0]), nearest_index(g.shape[1], out_hw[1])
    return class_index(g[ys][:, xs], n_class, colours)


def shuffle_order(n, draws):
    """the emissions of a shuffle buffer of size n over the stream 0, 1, .. n-1, 0, 1, .. for the slot `draws`"""
    buf, nxt, out = list(range(n)), 0, []
    for slot in draws:
        out.append(buf[slot])
        buf[slot] = nxt
        nxt = (nxt + 1) % n
    return out
