"""The knob surface of the package is a fixed, documented list (no GPU).

Every LSR_* / LANGSPLAT_AMD_* environment variable read under langsplat_amd/ is named here and in the
table of DESIGN.md section 9, and the library has no -D build knobs.  Adding a variable means editing
CPP_KNOBS / PY_KNOBS and that table on purpose."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "langsplat_amd")
CSRC = os.path.join(PKG, "csrc")

CPP_KNOBS = {
    "LSR_HOST_TRACE", "LSR_RENDER_STATS", "LSR_BUCKET_TIMELINE", "LSR_RADIX_SMALL_MAX", "LSR_DEPTH_LSD",
    "LSR_MSD_BUCKETS", "LSR_MSD_ITEMS", "LSR_PLACED",
}
PY_KNOBS = {
    "LSR_PG_NATIVE_LAUNCH", "LSR_PG_ROT", "LSR_PG_DEFER", "LSR_DIST_BACKEND", "LSR_GRAPH_COLLECTIVE",
    "LSR_OFFLOAD_ARCH", "LSR_FUSED_TAIL", "LSR_LIB", "LSR_ALL_GRADS", "LSR_DIRECT_RCCL", "LANGSPLAT_AMD_FUSED",
}
_NAME = r"((?:LSR|LANGSPLAT_AMD)_[A-Z0-9_]+)"


def _sources(top, suffixes):
    for d, _, files in os.walk(top):
        for f in sorted(files):
            if f.endswith(suffixes):
                with open(os.path.join(d, f), encoding="utf-8") as fh:
                    yield os.path.join(d, f), fh.read()


def test_environment_reads_are_the_listed_ones():
    cpp = set()
    for _, text in _sources(CSRC, (".hip", ".h", ".cpp")):
        cpp |= set(re.findall(r'getenv\(\s*"' + _NAME + '"', text))
    py = set()
    for _, text in _sources(PKG, (".py",)):
        py |= set(re.findall(r'os\.environ(?:\.get\(|\[)\s*"' + _NAME, text))
    assert cpp == CPP_KNOBS
    assert py == PY_KNOBS


def test_every_knob_is_in_the_design_table():
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as fh:
        rows = [ln for ln in fh if ln.startswith("| `")]
    documented = {m.group(1) for ln in rows for m in [re.match(r"\| `" + _NAME + r"` \|", ln)] if m}
    assert CPP_KNOBS | PY_KNOBS <= documented, sorted((CPP_KNOBS | PY_KNOBS) - documented)


def test_no_build_knobs_in_csrc():
    bad = []
    for path, text in _sources(CSRC, (".hip", ".h", ".cpp")):
        lines = text.split("\n")
        for i, ln in enumerate(lines):
            m = re.match(r"\s*#\s*ifndef\s+(LSR_\w+)", ln)
            if not m:
                continue
            nxt = lines[i + 1] if i + 1 < len(lines) else ""
            guard = m.group(1).endswith("_H") and re.match(r"\s*#\s*define\s+" + m.group(1) + r"\s*$", nxt)
            if not guard:
                bad.append(f"{os.path.relpath(path, ROOT)}:{i + 1}: {ln.strip()}")
    assert not bad, bad
