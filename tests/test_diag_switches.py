"""CPU: the diagnostic environment switches are the ones DESIGN.md §10 lists, and Diag::read is the only place that reads them."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libflate_amd", "csrc")


def _diag_read_body():
    src = open(os.path.join(CSRC, "lfx_api.cpp")).read()
    m = re.search(r"void Diag::read\(\) \{\n(.*?)\n\}\n", src, re.S)
    assert m, "Diag::read not found in lfx_api.cpp"
    return src, m


def test_switches_read_are_the_switches_documented():
    _src, m = _diag_read_body()
    read = set(re.findall(r'"(LFX_[A-Z0-9_]+)"', m.group(1)))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = re.search(r"\n## 10\. Diagnostics\n(.*?)\n## ", design, re.S)
    assert sec, "DESIGN.md §10 not found"
    # the list: from "Environment switches, read once ..." to the sentence that closes it
    lst = re.search(r"Environment switches, read once(.*?)Nothing else in", sec.group(1), re.S)
    assert lst, "DESIGN.md §10: the switch list not found"
    listed = set(re.findall(r"LFX_[A-Z0-9_]+", lst.group(1)))
    assert read == listed, (sorted(read - listed), sorted(listed - read))


def test_no_getenv_outside_diag_read():
    src, m = _diag_read_body()
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if not path.endswith((".h", ".hip", ".cpp", ".inc")):
            continue
        text = open(path).read()
        if os.path.basename(path) == "lfx_api.cpp":
            text = src[:m.start(1)] + src[m.end(1):]
        assert "getenv(" not in text, os.path.basename(path)
