"""Host: the exact-fp32 precision is declared where a caller looks for it -- the C header and the ctypes constants."""
import os
import re

from wsscam import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prec_f32_constant_matches_the_header():
    assert _lib.PREC_F32 == 4
    header = open(os.path.join(ROOT, "include", "wsscam.h")).read()
    enum = re.search(r"typedef enum wsc_precision \{(.*?)\} wsc_precision;", header, re.S).group(1)
    values = dict((n, int(v)) for n, v in re.findall(r"(WSC_PREC_\w+)\s*=\s*(\d+)", enum))
    assert values == {"WSC_PREC_BF16": _lib.PREC_BF16, "WSC_PREC_BF16X3": _lib.PREC_BF16X3, "WSC_PREC_F16": _lib.PREC_F16,
                      "WSC_PREC_F16X3": _lib.PREC_F16X3, "WSC_PREC_F32": _lib.PREC_F32}


def test_range_error_names_the_exact_fallback():
    header = open(os.path.join(ROOT, "include", "wsscam.h")).read()
    err = re.search(r"WSC_ERR_RANGE = -9(.*?)\*/", header, re.S).group(1)
    assert "65504" in err and "WSC_PREC_F32" in err
