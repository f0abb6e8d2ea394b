"""Device snapshots, the CPU side: the state inventory of h_snapshot.hip against the arrays the handle owns, the ctypes binding
against the header, and the resources of snapshot_copy_kernel.  (The GPU side is tests/test_snapshot.py.)

The inventory guard is written in the manner of test_gpu_variants.test_every_reported_kernel_has_a_row: it reads the sources.  Every
array that Upload::state_arrays, ensure_rss, ensure_rssq, ensure_wide and the front of episode_layout allocate must be named either
in the segment table of h_snapshot.hip (state: saved and restored) or in the kScratch list beside it (with its "scratch, because
..."); an array somebody adds later fails here until somebody decides which it is.
"""
import ctypes as C
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scenario_gym_amd", "csrc")
SYMBOLS = ("sg_snapshot_create", "sg_snapshot_save", "sg_snapshot_restore", "sg_snapshot_bytes", "sg_snapshot_destroy")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _body(src, head):
    """The text of the function whose definition starts with `head`, braces matched."""
    i = src.index(head)
    i = src.index("{", i)
    depth, j = 1, i + 1
    while depth:
        depth += {"{": 1, "}": -1}.get(src[j], 0)
        j += 1
    return src[i:j]


def owned_arrays():
    """The arrays between two calls of a handle, as the sources allocate them today."""
    names = re.findall(r"dev_alloc\(h, M, &(p\.\w+)", _body(_src("h_upload.hip"), "int Upload::state_arrays()"))
    names += ["wide_args." + n for n in re.findall(r"&h->wide_args\.(\w+)", _body(_src("h_wide.hip"), "int sgh::ensure_wide("))]
    names += re.findall(r"hipMalloc\(\(void \*\*\)&h->(d_rss\w+)", _body(_src("h_rss.hip"), "int sgh::ensure_rss("))
    names += re.findall(r"hipMalloc\(\(void \*\*\)&h->(d_rssq\w*)", _body(_src("h_rss.hip"), "int sgh::ensure_rssq("))
    layout = _body(_src("h_episode.hip"), "int sgh::episode_layout(")
    front = layout[:layout.index("+ state;")]  # (the accounting: what lies before the arrays of the view)
    names += re.findall(r"take\(a\.(\w+),", front)
    names += ["h->d_ext", "sg_episode_view", "qwords", "d_qtab", "d_tab", "slice_allocs"]  # the rest of the issue's inventory
    return names


def decided(src):
    state = re.findall(r'\bb\.seg\("([^"]+)"', src)
    scratch = re.findall(r'\{"([^"]+)",\s*"scratch, because [^"]{20,}"\}', src)
    return state, scratch


def undecided(names, src):
    state, scratch = decided(src)
    return [n for n in names if n not in state and n not in scratch]


def test_every_owned_array_is_state_or_scratch():
    names = owned_arrays()
    for must in ("p.dyn", "p.sdyn", "p.events", "p.ev_pose", "p.ev_hpose", "p.rec_t", "p.rec_pose", "p.ctl_state", "wide_args.last_row",
                 "wide_args.last_same", "wide_args.scr", "wide_args.dup", "d_rss_state", "d_rss_seen", "d_rssq", "prev_s", "acc_return",
                 "acc_length", "prev_ok"):
        assert must in names, f"the parse lost {must}: {names}"  # (the parse found what is there today)
    assert len(names) == len(set(names))
    src = _src("h_snapshot.hip")
    state, scratch = decided(src)
    assert not undecided(names, src), f"neither saved by a snapshot nor listed as scratch: {undecided(names, src)}"
    assert not set(state) & set(scratch)
    assert set(state) | set(scratch) <= set(names), "h_snapshot.hip names an array the handle does not own"
    # ... and the check does bite: without its line, an array is named
    for gone in ('b.seg("p.sdyn"', 'b.seg("prev_ok"', '{"p.ctl_state"', '{"wide_args.dup"'):
        assert gone in src
        name = re.search(r'"([^"]+)"', gone).group(1)
        assert undecided(names, src.replace(gone, "(")) == [name]


def test_binding_matches_the_header():
    """_lib binds the five symbols with the argument types the header declares."""
    sys.path.insert(0, ROOT)
    import scenario_gym_amd._lib as L

    with open(os.path.join(ROOT, "include", "sgym.h")) as f:
        header = f.read()
    ctype = {"sg_handle *": C.c_void_p, "sg_snapshot *": C.c_void_p, "const sg_snapshot *": C.c_void_p, "sg_snapshot **": C.POINTER(C.c_void_p),
             "const uint8_t *": C.c_void_p, "int32_t": C.c_int32, "uint64_t *": C.POINTER(C.c_uint64)}
    lib = L.load()
    for name in SYMBOLS:
        assert name in L.SYMBOLS
        m = re.search(r"^int %s\(([^)]*)\);" % name, header, re.M)
        assert m, name
        want = []
        for arg in m.group(1).split(","):
            t = re.match(r"\s*(.*?)(\w+)\s*$", arg).group(1).strip()
            want.append(ctype[t])
        fn = getattr(lib, name)
        assert list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is C.c_int or fn.restype is C.c_int32
    assert "typedef struct sg_snapshot sg_snapshot;" in header and "#define SG_ABI_VERSION 7 " in header
    assert all(n in header.split("#define SG_ABI_VERSION 7", 1)[1].split("*/", 1)[0] for n in SYMBOLS)  # (the "added within 7" list)


def test_copy_kernel_resources():
    """snapshot_copy_kernel is a streaming copy: no scratch, no LDS, and few enough registers for eight wavefronts per SIMD.  Read
    from the built code object."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import table

    rows = {n: r for n, r in table().items() if "snapshot_copy_kernel" in n}
    assert len(rows) == 1, list(rows)
    (r,) = rows.values()
    assert r["scratch"] == 0 and r["lds"] == 0 and r["vgpr"] + r["agpr"] <= 64, r
