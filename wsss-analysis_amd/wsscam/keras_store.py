"""What the Keras-era drivers (02_cues/demo.py, 03c_hsn/demo.py) load from disk before their batch loops, for callers that
do not hand the loaded objects in: `settings.ini`, the classifier CNN of a session (`<sess_id>.h5` weights + `<sess_id>.mat`
thresholds under MODEL_ROOT/<dataset>_<model_type>/) and the image list + image-level labels of a split (the CSV files the
reference's `Dataset` class feeds to Keras' flow_from_dataframe, 02_cues/dataset.py:98-124).

The device networks have the two fixed conv tables of the reference's torch mirrors (net/vgg16.py:44, net/m7.py:41), selected
by `model_type` -- 'VGG16*' -> modified VGG16, 'M7*' / 'X1.7' -> M7.  A session's `<sess_id>.json` (Keras 2 `model.to_json()`,
what the reference hands to model_from_json) is read when it lies beside the `.h5`: `read_architecture` checks its layer
sequence against that table -- any other layer, order, kernel, activation placement or BatchNorm epsilon is a ValueError, never
a fallback -- and takes from it what the table leaves open, the geometry of the MaxPooling2D layers, which `load_model` sets
on the model (`set_pooling`) before the network is packed and before the Grad-CAM weights are computed.  With no `.json` on
disk the pools are the torch port's MaxPool2d(2, 2), exactly as before.
Reading `.h5` needs h5py (net.common.keras_h5_weight_list); a missing file or module is an error, never a fallback."""
import configparser
import csv
import os

import numpy as np

VOC_CLASSES = ["aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog",
               "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor"]
DEEPGLOBE_CLASSES = ["urban", "agriculture", "rangeland", "forest", "water", "barren", "unknown"]
ADP_CLASSES = ["E.M.S", "E.M.U", "E.M.O", "E.T.S", "E.T.U", "E.T.O", "E.P", "C.D.I", "C.D.R", "C.L", "H.E", "H.K", "H.Y", "S.M.C",
               "S.M.S", "S.E", "S.C.H", "S.R", "A.W", "A.B", "A.M", "M.M", "M.K", "N.P", "N.R.B", "N.R.A", "N.G.M", "N.G.W", "G.O",
               "G.N", "T"]


def read_settings(path=None):
    """02_cues/demo.py:16-24 / 03c_hsn/demo.py: `../settings.ini` relative to the working directory (WSSCAM_SETTINGS overrides)."""
    path = path or os.environ.get("WSSCAM_SETTINGS", os.path.join("..", "settings.ini"))
    cfg = configparser.ConfigParser()
    if not cfg.read(path):
        raise FileNotFoundError("settings file %s not found (pass the loaded objects, or set WSSCAM_SETTINGS)" % path)
    data = cfg["Download Directory"]["data_dir"]
    if not os.path.isabs(data):  # relative to the working directory, as the reference's os.path.join(...) use of it is
        data = os.path.normpath(os.path.join(os.getcwd(), data))
    return {"DATA_ROOT": data, "MODEL_ROOT": os.path.join(data, cfg["Data Folders"]["model_cnn_dir"]),
            "CUES_ROOT": os.path.join(data, cfg["Data Folders"]["cues_dir"])}


def read_option(path, key, default):
    """An optional key of settings.ini's [Data Folders] section (keys the reference's file does not have: defaults apply)."""
    path = path or os.environ.get("WSSCAM_SETTINGS", os.path.join("..", "settings.ini"))
    cfg = configparser.ConfigParser()
    if not cfg.read(path):
        raise FileNotFoundError(path)
    return cfg["Data Folders"].get(key, default) if cfg.has_section("Data Folders") else default


class SetList:
    """The three attributes the drivers read off a Keras DataFrameIterator: `directory`, `filenames`, `data` (labels)."""

    def __init__(self, directory, filenames, data):
        self.directory, self.filenames, self.data = directory, list(filenames), np.asarray(data)

    def images(self, lo=0, hi=None):
        from PIL import Image

        return [np.asarray(Image.open(os.path.join(self.directory, f)).convert("RGB")) for f in self.filenames[lo:hi]]


class Dataset:
    """02_cues/dataset.py:5-124 / 03c_hsn/dataset.py:5-124 without the Keras generators: per split the image directory, the
    file names ('Patch Names' column) and the label matrix (the class-name columns) of
    <devkit>/ImageSets/Segmentation/<split>.csv, in file order (the evaluation generators are not shuffled; the drivers only
    read `.filenames` / `.data` of the training one).

    The two reference classes differ, selected by `layout`:
      * "cues" (02_cues/dataset.py): `database_dir` is ALWAYS <parent of the working directory>/database (:12 -- the class
        takes no directory argument; an explicit `database_dir` here is an override for callers with another tree);
        VOC2012 = VOCdevkit/VOC2012 with ['trainaug', 'val']; DeepGlobe names 'DeepGlobe_train75' / 'DeepGlobe_train37.5'
        (the drivers' 'DeepGlobe' / 'DeepGlobe_balanced' are accepted as aliases of the two);
      * "hsn" (03c_hsn/dataset.py): `database_dir` is the DATA_ROOT argument (:8, demo.py:88); VOC2012 =
        VOCdevkit/VOC_trainaug_val/VOC2012 with the 'val' split only (:57-59); DeepGlobe names 'DeepGlobe' (train75) /
        'DeepGlobe_balanced' (train37.5) (:84-89)."""

    def __init__(self, data_type="ADP", size=321, batch_size=16, database_dir=None, layout="cues"):
        if layout not in ("cues", "hsn"):
            raise ValueError("layout must be 'cues' or 'hsn'")
        if layout == "hsn" and database_dir is None:
            raise ValueError("the 03c_hsn Dataset takes its database_dir argument (DATA_ROOT), there is no default")
        self.data_type, self.size, self.batch_size, self.layout = data_type, size, batch_size, layout
        self.database_dir = database_dir or os.path.join(os.path.dirname(os.getcwd()), "database")
        if data_type == "ADP":
            self.devkit_dir = os.path.join(self.database_dir, "ADPdevkit", "ADPRelease1")
            self.sets, self.is_evals, self.class_names = ["valid", "test"], [True, True], list(ADP_CLASSES)
        elif data_type == "VOC2012":
            if layout == "hsn":
                self.devkit_dir = os.path.join(self.database_dir, "VOCdevkit", "VOC_trainaug_val", "VOC2012")
                self.sets, self.is_evals = ["val"], [True]
            else:
                self.devkit_dir = os.path.join(self.database_dir, "VOCdevkit", "VOC2012")
                self.sets, self.is_evals = ["trainaug", "val"], [False, True]
            self.class_names = list(VOC_CLASSES)
        elif "DeepGlobe" in data_type:
            self.devkit_dir = os.path.join(self.database_dir, "DGdevkit")
            names = {"DeepGlobe": "train75", "DeepGlobe_balanced": "train37.5"}
            if layout == "cues":
                names.update({"DeepGlobe_train75": "train75", "DeepGlobe_train37.5": "train37.5"})
            train = names.get(data_type)
            if train is None:
                raise ValueError("unknown DeepGlobe data_type %r" % data_type)
            self.sets, self.is_evals, self.class_names = [train, "test"], [False, True], list(DEEPGLOBE_CLASSES)
        else:
            raise ValueError("unknown data_type %r" % data_type)
        img_folder = "PNGImages" if data_type == "ADP" else "JPEGImages"
        self.set_gens = {}
        for s in self.sets:
            with open(os.path.join(self.devkit_dir, "ImageSets", "Segmentation", s + ".csv"), newline="") as f:
                rows = list(csv.DictReader(f))
            self.set_gens[s] = SetList(os.path.join(self.devkit_dir, img_folder), [r["Patch Names"] for r in rows],
                                       np.array([[float(r[c]) for c in self.class_names] for r in rows], dtype=np.float32)
                                       .reshape(len(rows), len(self.class_names)))


def _square(v, what, i):
    """An int, or a pair of equal ints, of a Keras layer config -> the int."""
    if isinstance(v, (list, tuple)):
        if len(v) != 2 or v[0] != v[1]:
            raise ValueError("layer %d: %s %r is not square" % (i, what, v))
        v = v[0]
    if not isinstance(v, int) or isinstance(v, bool):
        raise ValueError("layer %d: %s %r is not an integer" % (i, what, v))
    return v


def read_architecture(path, model_type):
    """The session's architecture file -> (pooling, has_batchnorm): pooling = [(k, stride, 'same' | 'valid'), ...] of the
    MaxPooling2D layers in the order they occur (for M7 the classifier branch's pool last), as the CAM wrappers' `pooling` takes it.

    `path` holds Keras 2 `model.to_json()` of a Sequential model, `"config"` either the layer list or `{"layers": [...]}`.
    InputLayer and Dropout entries are skipped; the rest must be the model type's table (net.common.PLAIN_CFG):
    per conv entry Conv2D(filters, 3 x 3, stride 1, 'same', linear) -> Activation('relu') [-> BatchNormalization(epsilon 1e-3):
    after every Activation or after none], MaxPooling2D at the 'M' positions (and, M7, before the global pooling),
    GlobalAveragePooling2D (VGG16) / GlobalMaxPooling2D (M7), Dense with the model type's use_bias, optionally a final
    Activation('sigmoid').  Anything else raises ValueError with the layer's index and what was expected there -- a ReLU fused
    into the Conv2D included: find_final_layer would then name the BatchNorm, another Grad-CAM contraction point."""
    import json

    from .net.common import PLAIN_CFG, normalize_pooling

    root = "vgg16" if "VGG16" in model_type else "m7"
    with open(path) as f:
        doc = json.load(f)
    if not isinstance(doc, dict) or doc.get("class_name") != "Sequential":
        raise ValueError("%s: a Keras Sequential model is expected, got class_name %r" %
                         (path, doc.get("class_name") if isinstance(doc, dict) else type(doc).__name__))
    cfg = doc.get("config")
    if isinstance(cfg, dict):
        cfg = cfg.get("layers")
    if not isinstance(cfg, list):
        raise ValueError("%s: no layer list under 'config'" % path)
    layers = [(i, l.get("class_name"), l.get("config") or {}) for i, l in enumerate(cfg)
              if l.get("class_name") not in ("InputLayer", "Dropout")]
    pos = [0]

    def take(expected):
        if pos[0] >= len(layers):
            raise ValueError("%s: the model ends after %d layers where %s was expected" % (path, len(cfg), expected))
        i, name, c = layers[pos[0]]
        if name != expected:
            raise ValueError("%s: layer %d is %s, expected %s" % (path, i, name, expected))
        pos[0] += 1
        return i, c

    def peek():
        return layers[pos[0]][1] if pos[0] < len(layers) else None

    def max_pool():
        i, c = take("MaxPooling2D")
        k = _square(c.get("pool_size"), "pool_size", i)
        stride = k if c.get("strides") is None else _square(c.get("strides"), "strides", i)
        padding = c.get("padding")
        if k not in (2, 3) or stride not in (1, 2) or stride > k or padding not in ("same", "valid"):
            raise ValueError("%s: layer %d: MaxPooling2D(%r, strides %r, %r) -- window 2 / 3, stride 1 / 2 (<= window), 'same' / "
                             "'valid' are supported" % (path, i, k, stride, padding))
        return k, stride, padding

    pooling, has_bn = [], None
    for _, table in PLAIN_CFG[root]:
        for v in table:
            if v == "D":
                continue
            if v == "M":
                pooling.append(max_pool())
                continue
            i, c = take("Conv2D")
            if c.get("filters") != v:
                raise ValueError("%s: layer %d: Conv2D with %r filters, expected %d" % (path, i, c.get("filters"), v))
            if _square(c.get("kernel_size"), "kernel_size", i) != 3 or _square(c.get("strides", 1), "strides", i) != 1 \
                    or c.get("padding") != "same" or _square(c.get("dilation_rate", 1), "dilation_rate", i) != 1:
                raise ValueError("%s: layer %d: Conv2D must be 3 x 3, stride 1, padding 'same', got kernel %r strides %r padding %r"
                                 % (path, i, c.get("kernel_size"), c.get("strides"), c.get("padding")))
            if c.get("activation", "linear") != "linear":
                raise ValueError("%s: layer %d: Conv2D with a fused %r activation, expected a linear Conv2D followed by an "
                                 "Activation layer" % (path, i, c.get("activation")))
            if c.get("use_bias", True) is not True:
                raise ValueError("%s: layer %d: Conv2D without a bias" % (path, i))
            i, c = take("Activation")
            if c.get("activation") != "relu":
                raise ValueError("%s: layer %d: Activation %r, expected 'relu'" % (path, i, c.get("activation")))
            bn = peek() == "BatchNormalization"
            if has_bn is None:
                has_bn = bn
            elif bn != has_bn:
                raise ValueError("%s: layer %d: BatchNormalization must follow every Activation or none"
                                 % (path, layers[min(pos[0], len(layers) - 1)][0]))
            if bn:
                i, c = take("BatchNormalization")
                if abs(float(c.get("epsilon", 1e-3)) - 1e-3) > 1e-9:
                    raise ValueError("%s: layer %d: BatchNormalization epsilon %r, expected 1e-3" % (path, i, c.get("epsilon")))
    if root == "m7":
        pooling.append(max_pool())  # layer3_p2 of the classifier branch (net/m7.py:15-21)
    take("GlobalAveragePooling2D" if root == "vgg16" else "GlobalMaxPooling2D")
    i, c = take("Dense")
    use_bias = "VGG16" not in model_type  # common_cnn.py:44
    if bool(c.get("use_bias", True)) != use_bias:
        raise ValueError("%s: layer %d: Dense use_bias %r, a %s model has %r" % (path, i, c.get("use_bias"), model_type, use_bias))
    if c.get("activation", "linear") not in ("linear", "sigmoid"):
        raise ValueError("%s: layer %d: Dense activation %r, expected 'sigmoid' (or linear + Activation)" % (path, i, c.get("activation")))
    if peek() == "Activation":
        i, c = take("Activation")
        if c.get("activation") != "sigmoid":
            raise ValueError("%s: layer %d: Activation %r after the Dense layer, expected 'sigmoid'" % (path, i, c.get("activation")))
    if pos[0] != len(layers):
        raise ValueError("%s: layer %d is %s, expected the end of the model" % (path, layers[pos[0]][0], layers[pos[0]][1]))
    return normalize_pooling(pooling), bool(has_bn)


def read_dropout(path, model_type):
    """The `rate` of the Dropout layers of a session's architecture file (the format read_architecture takes) -> a float, or None
    if the file has no Dropout layer (such a session was trained without).  The model type's table has net.common.DROP_SITES of
    them (VGG16: two in layer5; M7: one behind layer3_p2) and nn.Dropout(p=0.5) at each; any other count, or sites whose rates
    disagree, raise ValueError with the layer's index: ClsTrainer has ONE drop_prob for all sites.  The value is what
    cls_train.train(drop_prob=...) takes; the masks are the project's own, not Keras' stream."""
    import json

    from .net.common import DROP_SITES

    root = "vgg16" if "VGG16" in model_type else "m7"
    with open(path) as f:
        doc = json.load(f)
    cfg = doc.get("config") if isinstance(doc, dict) else None
    if isinstance(cfg, dict):
        cfg = cfg.get("layers")
    if not isinstance(cfg, list):
        raise ValueError("%s: no layer list under 'config'" % path)
    found = [(i, (l.get("config") or {}).get("rate")) for i, l in enumerate(cfg) if l.get("class_name") == "Dropout"]
    if not found:
        return None
    if len(found) != DROP_SITES[root]:
        i = found[min(len(found), DROP_SITES[root] + 1) - 1][0]
        raise ValueError("%s: layer %d: %d Dropout layers, a %s model has %d" % (path, i, len(found), model_type, DROP_SITES[root]))
    for i, rate in found:
        if isinstance(rate, bool) or not isinstance(rate, (int, float)) or not 0.0 <= rate < 1.0:
            raise ValueError("%s: layer %d: Dropout rate %r (0 <= rate < 1)" % (path, i, rate))
        if float(rate) != float(found[0][1]):
            raise ValueError("%s: layer %d: Dropout rate %r, layer %d has %r -- one rate for every site is supported"
                             % (path, i, rate, found[0][0], found[0][1]))
    return float(found[0][1])


def load_model(model_dir, sess_id, model_type, dataset, device=0, precision=None):
    """02_cues/demo.py:104-124 / 03c_hsn/utilities.py build_model + load_thresholds + get_grad_cam_weights:
    (device CAM wrapper with the session's weights, alpha (F, C), final layer name, thresholds (1, C))."""
    import scipy.io

    from .cues import utilities as cu
    from .net import m7_cam, vgg16_cam
    from .net.common import keras_h5_weight_list, state_dict_from_keras_weights

    cls = vgg16_cam.CAM if "VGG16" in model_type else m7_cam.CAM
    thresholds = scipy.io.loadmat(os.path.join(model_dir, sess_id + ".mat")).get("optimalScoreThresh")
    weights = keras_h5_weight_list(os.path.join(model_dir, sess_id + ".h5"))
    num_classes = int(np.asarray(thresholds).shape[1])
    ds_tag = {"ADP": "adp_morph", "VOC2012": "voc12"}.get(dataset, "deepglobe")
    model = cls(None, ds_tag, model_type, num_classes, None, precision=precision)
    arch_path = os.path.join(model_dir, sess_id + ".json")
    if os.path.exists(arch_path):  # the session's own pools: before the net is packed and before alpha (its map size)
        pooling, has_bn = read_architecture(arch_path, model_type)
        if has_bn != bool(model.batchnorm):
            raise ValueError("%s: the architecture %s BatchNorm, the %s / %s model type %s" % (
                arch_path, "has" if has_bn else "has no", dataset, model_type, "has it" if model.batchnorm else "has none"))
        model.set_pooling(pooling)
    model.load_state_dict(state_dict_from_keras_weights(weights, model_type, cls.root, model.batchnorm, np.asarray(thresholds)[0]))
    model.cuda(device)
    img_size = 321 if model_type in ("VGG16", "VGG16bg") else 224
    final_layer = cu.find_final_layer(model)
    alpha = cu.get_grad_cam_weights(model, final_layer, np.zeros((1, img_size, img_size, 3)))
    return model, alpha, final_layer, np.asarray(thresholds)


def fgbg_sessions(model_dir, sess_id, fgbg_modes):
    """02_cues/demo.py:139-150: where the background model of a VOC2012 session lives."""
    out = {}
    for m in fgbg_modes:
        if m == "fg":
            out[m] = (model_dir, sess_id)
        elif "fg" in sess_id:
            out[m] = (model_dir.replace("fg", "bg"), sess_id.replace("fg", "bg"))
        else:
            out[m] = (model_dir.replace("fg", "") + "bg", sess_id.replace("fg", "") + "bg")
    return out
