"""TEST INFRASTRUCTURE ONLY -- loads ONE file of the reference tree as a module although packages it imports are absent.

    mod = ref_import.load("02_cues/utilities.py")         # the reference's own get_fgbg_cues, run as it stands
    mod = ref_import.load("03b_irn/net/resnet50_irn.py", with_dir="03b_irn")

The file is loaded by path under a unique module name (`utilities.py` exists four times in the reference).  Before the load, a
stub module is installed for every ABSENT package of STUB_ROOTS (keras, cv2, tensorflow, ..., and the reference's own missing
`misc`, `lib`, `model_loader`, `data_loader`); a package that is installed is used as it is.  A stub lets `import a.b as K`
and `from a.b import name` succeed and nothing else: a stub module, and every name imported from one, raises RuntimeError
naming the attribute on any non-dunder attribute access, on a call, on iteration and on indexing -- a fixture can never
silently depend on a stand-in.  After the load `sys.modules`, `sys.path`, `sys.meta_path` and the working directory are what
they were before; the stubs stay reachable only through the loaded module's own globals, where they go on raising.

ONE DELIBERATE STAND-IN: `lib.CC_labeling_8.CC_lab` (CCLabStandIn below).  The file is not in the reference tree; the stand-in
has its `labels` / `connectedComponentLabel()` interface over scipy.ndimage.label with a full 3 x 3 structure, so the
CONNECTIVITY of 03a_sec-dsrg/DSRG.py stays unpinned.

Nothing of the reference's text is copied: it is read at generation time only (oracle/gen_golden_ref.py), as oracle/gen_golden.py
does.  Regenerate the fixtures with `python oracle/gen_golden_ref.py all`."""
import contextlib
import importlib.abc
import importlib.machinery
import importlib.util
import itertools
import os
import sys
import types

REFERENCE_ROOT = os.environ.get("WSC_REFERENCE_ROOT", "/root/reference")

STUB_ROOTS = ("keras", "cv2", "tensorflow", "skimage", "pydensecrf", "imageio", "chainercv", "misc", "lib", "model_loader",
              "data_loader", "h5py", "torchvision")

_counter = itertools.count()


def available():
    return os.path.isdir(REFERENCE_ROOT)


def _refuse(owner, name):
    raise RuntimeError("stub %r: attribute %r was touched -- this module is absent here and must not be reached" % (owner, name))


class StubAttr:
    """What `from <stub> import name` binds: any use raises."""

    def __init__(self, qualname):
        object.__setattr__(self, "_stub_qualname", qualname)

    def __getattr__(self, name):
        if name.startswith("__") and name.endswith("__"):
            raise AttributeError(name)
        _refuse(object.__getattribute__(self, "_stub_qualname"), name)

    def __call__(self, *a, **k):
        _refuse(object.__getattribute__(self, "_stub_qualname"), "__call__")

    def __iter__(self):
        _refuse(object.__getattribute__(self, "_stub_qualname"), "__iter__")

    def __getitem__(self, key):
        _refuse(object.__getattribute__(self, "_stub_qualname"), "__getitem__")

    def __mro_entries__(self, bases):
        _refuse(object.__getattribute__(self, "_stub_qualname"), "__mro_entries__")

    def __repr__(self):
        return "<stub attribute %s>" % object.__getattribute__(self, "_stub_qualname")


class StubModule(types.ModuleType):
    """A module of an absent package.  While its load is going on, `from stub import name` binds a StubAttr (the import
    statement itself must succeed); once sealed, every non-dunder attribute access raises."""

    def __init__(self, name):
        super().__init__(name)
        self.__dict__["__path__"] = []  # a package: `import stub.sub` asks the finder
        self.__dict__["__all__"] = []   # `from stub import *` binds nothing
        self.__dict__["_stub_state"] = {"sealed": False}

    def __getattr__(self, name):
        if name.startswith("__") and name.endswith("__"):
            raise AttributeError(name)
        if self.__dict__["_stub_state"]["sealed"]:
            _refuse(self.__name__, name)
        return StubAttr(self.__name__ + "." + name)


class CCLabStandIn:
    """STAND-IN for lib/CC_labeling_8.py::CC_lab, which is not in the reference tree: `labels` is a list of lists of component
    numbers (0 outside the mask), 8-connected by scipy.ndimage.label with a full 3 x 3 structure."""

    def __init__(self, mat):
        self.mat = mat
        self.labels = [[0] * len(row) for row in mat]

    def connectedComponentLabel(self):
        import numpy as np
        import scipy.ndimage

        lab, _ = scipy.ndimage.label(np.asarray(self.mat) != 0, structure=np.ones((3, 3), int))
        self.labels = lab.tolist()


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def __init__(self, roots):
        self.roots = set(roots)
        self.made = []

    def find_spec(self, fullname, path=None, target=None):
        if fullname.split(".")[0] in self.roots:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        mod = StubModule(spec.name)
        self.made.append(mod)
        return mod

    def exec_module(self, module):
        if module.__name__ == "lib.CC_labeling_8":
            module.__dict__["CC_lab"] = CCLabStandIn  # the one deliberate stand-in


def absent_roots(extra_path=()):
    """The STUB_ROOTS that cannot be imported here (with `extra_path` in front of sys.path)."""
    saved = list(sys.path)
    sys.path[:0] = list(extra_path)
    try:
        out = []
        for root in STUB_ROOTS:
            if root in sys.modules and not isinstance(sys.modules[root], StubModule):
                continue
            try:
                found = importlib.util.find_spec(root) is not None
            except (ImportError, ValueError):
                found = False
            if not found:
                out.append(root)
        return out
    finally:
        sys.path[:] = saved


@contextlib.contextmanager
def _restored(root):
    """sys.path and sys.meta_path come back exactly as they were.  sys.modules: every entry that was there is there again (the
    same object), and no stub and no module of the reference tree stays behind.  Installed packages that the reference file
    imported for the first time (scipy, sklearn, pandas, ...) stay imported: unloading them would make a later import load a
    second copy."""
    modules, path, meta, cwd = dict(sys.modules), list(sys.path), list(sys.meta_path), os.getcwd()
    root = os.path.realpath(root) + os.sep
    try:
        yield
    finally:
        os.chdir(cwd)
        for k, m in list(sys.modules.items()):
            if k in modules:
                continue
            src = [getattr(m, "__file__", None)] + list(getattr(m, "__path__", None) or [])  # (a namespace package has no file)
            if isinstance(m, StubModule) or k.startswith("_wsc_ref_") or \
                    any(os.path.realpath(s).startswith(root) for s in src if isinstance(s, str)):
                del sys.modules[k]
        sys.modules.update(modules)
        sys.path[:] = path
        sys.meta_path[:] = meta


def load(rel_path, with_dir=None, root=None):
    """Load `<reference>/<rel_path>` as a module.  with_dir: a directory (relative to the reference root; True = the file's own)
    that is put in front of sys.path for this load only, for files that import their siblings (`from utilities import *`,
    `from net import resnet50`).  Sibling modules loaded on the way leave sys.modules again with everything else."""
    root = REFERENCE_ROOT if root is None else root
    path = os.path.join(root, rel_path)
    if not os.path.isfile(path):
        raise FileNotFoundError(path)
    extra = []
    if with_dir is True:
        extra = [os.path.dirname(path)]
    elif with_dir:
        extra = [os.path.join(root, with_dir)]
    name = "_wsc_ref_%d_%s" % (next(_counter), "".join(c if c.isalnum() else "_" for c in rel_path))
    finder = _StubFinder(absent_roots(extra))
    with _restored(root):
        siblings = {os.path.splitext(f)[0] for d in extra for f in os.listdir(d)}  # `import utilities` must find THIS directory's
        for k in [k for k in sys.modules if k.split(".")[0] in finder.roots | siblings]:
            del sys.modules[k]
        sys.path[:0] = extra
        if extra:
            os.chdir(extra[0])  # (voc12/dataloader.py reads 'voc12/cls_labels.npy' relative to 03b_irn while it is imported)
        sys.meta_path.insert(0, finder)
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        try:
            spec.loader.exec_module(mod)
        finally:
            for stub in finder.made:
                stub.__dict__["_stub_state"]["sealed"] = True
    mod.__dict__["_wsc_stubbed"] = sorted(m.__name__ for m in finder.made)
    return mod


def line_range(obj):
    """'first-last' source lines of a function or class of a loaded module"""
    import inspect

    if inspect.isclass(obj):  # (the loaded module has left sys.modules, which inspect needs for a class: span its methods)
        spans = [line_range(f).split("-") for f in vars(obj).values() if inspect.isfunction(f)]
        return "%d-%d" % (min(int(a) for a, _ in spans), max(int(b) for _, b in spans))
    lines, first = inspect.getsourcelines(obj)
    return "%d-%d" % (first, first + len(lines) - 1)
