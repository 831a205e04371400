"""Static check (no GPU, no build): every DevBuf the library declares -- struct member or local -- is classified in
csrc/scratch_list.hpp, either visited by for_each_scratch (its content is poisoned between calls by the scratch-reuse tests,
tests/test_gpu_scratch_reuse.py) or named in the header's list of caches and call-local buffers.  A buffer added later cannot
stay out of both lists unnoticed."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "algebra_amd", "csrc")
LIST = os.path.join(CSRC, "scratch_list.hpp")


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def declared_devbufs():
    """{name: [file, ...]} of every variable or member whose type is DevBuf, DevBuf&, DevBuf* or a map onto DevBuf"""
    found = {}
    files = [f for pat in ("*.hpp", "*.cuh", "*.hip") for f in glob.glob(os.path.join(CSRC, pat))]
    assert len(files) > 30
    for f in sorted(files):
        if os.path.samefile(f, LIST):
            continue
        code = strip_comments(open(f).read())
        names = []
        # DevBuf a, b[2], c;   DevBuf& r = ...;   DevBuf* p;      (declarations end in ';', parameters do not)
        for m in re.finditer(r"\bDevBuf\b\s*[&*]?\s*([A-Za-z_][\w\s,\[\]]*?)\s*(?:=[^;]*)?;", code):
            names += [re.sub(r"\[.*", "", n).strip() for n in m.group(1).split(",")]
        # std::map<Key, DevBuf> name;
        names += re.findall(r"\bDevBuf\s*>\s*(\w+)\s*;", code)
        for n in names:
            assert re.fullmatch(r"[A-Za-z_]\w*", n), (f, n)
            found.setdefault(n, []).append(os.path.basename(f))
    return found


def classified():
    text = open(LIST).read()
    body = text[text.index("void for_each_scratch("):text.index("void for_each_pinned_scratch(")]
    body = "\n".join(l for l in body.splitlines() if not l.startswith("#define"))   # (the macros' own parameter)
    scratch = {re.sub(r"\[.*", "", m).split(".")[-1] for m in re.findall(r"ARK_SCRATCH_(?:LANE|CTX)\(([\w.\[\]]+)\)", body)}
    scratch |= set(re.findall(r"c\.fft\.(\w+)\)", body))   # the per-stream ping buffers: a loop over the map
    caches, local = set(), set()
    for line in text.splitlines():
        m = re.match(r"//\s+cache:\s+(.*)", line)
        if m:
            caches |= set(re.findall(r"\b\w+::(\w+)", m.group(1).split(" -- ")[0].split("  ")[0]))
        m = re.match(r"//\s+local:\s+(\w+)", line)
        if m:
            local.add(m.group(1))
    return scratch, caches, local


def test_the_scan_finds_the_known_buffers():
    found = declared_devbufs()
    for known in ("keys", "lvlS", "lvlA", "nzcnt", "stage_a", "ring_s", "ring_b", "piece_buckets", "comm_sums", "tmps", "powers",
                  "roots9", "axis_pw", "dev", "table", "tmp", "poly_work", "pw"):
        assert known in found, known
    assert "msm.cuh" in found["keys"] and "fft.cuh" in found["tmps"] and "capi_core.hpp" in found["table"]


def test_every_devbuf_is_scratch_or_a_listed_cache():
    found = declared_devbufs()
    scratch, caches, local = classified()
    assert len(scratch) >= 40 and {"tmps", "keys", "cidx", "parts", "stage", "pw"} <= scratch, scratch
    assert {"roots", "roots9", "small", "tables", "powers", "axis_pw", "dev", "table"} <= caches, caches
    assert not (scratch & caches), scratch & caches
    missing = {n: fs for n, fs in found.items() if n not in scratch | caches | local}
    assert not missing, "DevBuf neither in for_each_scratch nor in the cache list of scratch_list.hpp: %r" % missing
    stale = (scratch | caches | local) - set(found) - {"tables"}   # (tables: a map onto FftTables, whose members are listed)
    assert not stale, "scratch_list.hpp names buffers the sources no longer declare: %r" % stale


def test_high_water_marks_are_recorded_and_nothing_reads_them():
    """DevBuf::asked and MsmJob::pinned_asked exist for the test hooks alone: outside msm.cuh's three lines each, only
    scratch_list.hpp and capi_test.hip may name them."""
    for f in glob.glob(os.path.join(CSRC, "*")):
        base = os.path.basename(f)
        if not base.endswith((".hpp", ".cuh", ".hip", ".h")) or base in ("msm.cuh", "scratch_list.hpp", "capi_test.hip"):
            continue
        code = strip_comments(open(f).read())
        assert not re.search(r"\b(pinned_asked|\.asked|->asked)\b", code), base
    msm = strip_comments(open(os.path.join(CSRC, "msm.cuh")).read())
    assert len(re.findall(r"\basked\b", msm)) == 4 and len(re.findall(r"\bpinned_asked\b", msm)) == 4, "msm.cuh"
    assert re.search(r"int ensure\(size_t bytes\) \{\s*if \(bytes > asked\) asked = bytes;\s*if \(bytes <= cap\) return 0;", msm)
