"""The argument rules of the point-cloud and held-object entries of the C boundary, all of them through ONE table: the code every
entry answers, and the ``nbk_last_error`` text it leaves, for each single fault, for nothing to do, for the size limits and for the
pairs of faults whose order decides the answer.  No device: the handles are stand-ins, and every case ends, at the latest, where
the entry asks whose the handles are.

Stand-ins (as tests/test_held_cloud_host.py): ``m`` and ``c`` are 4096 bytes of 0x7f -- a descriptor "of device 2139062143" with
more than 256 robot shapes, so a cloud entry whose own rules are through answers INVALID with "descriptor belongs to device", on a
machine with a GPU as on one without --; ``held`` is zeroed memory, a held object "made against another descriptor" with no items;
every array is one 64-byte aligned address.

``nbk_last_error`` is never cleared, so a case that expects NO text runs behind a call that leaves a known one (SENTINEL) and
expects to find that one still there.

The rows of the table hold the three families side by side: the point cloud's entries (7), the held object's (8) and the held
object's against a cloud (7)."""
import ctypes as C

import numpy as np
import pytest

from numbotics_amd import _lib

nan, inf = float("nan"), float("inf")
OK, INVALID, UNSUPPORTED = 0, -1, -4
DEVICE, FOREIGN = "descriptor belongs to device 2139062143", "the held object was made against another descriptor"
HEAD = {"cloud": ("m", "c"), "held": ("m", "held"), "held_cloud": ("m", "held", "c")}
SEL = {"cloud": ("shape_bits",), "held": ("grasp",), "held_cloud": ("grasp",)}            # the slot in front of `accumulate`
GRASP = ("grasp", "grasp_rows")


def _order(family, kind):
    """-> the parameter names of the entry, in the order of include/nbk.h"""
    cloud = family == "cloud"
    look = () if family == "held" else ("look_ahead",)
    body = {
        "validity": ("q", "B") + (("threshold", "shape_bits") if cloud else GRASP + ("threshold",)) + ("accumulate", "mask_bits", "mask_bytes"),
        "clearance": ("q", "B") + (("d_max", "shape_bits") if cloud else GRASP + ("d_max",)) + ("min_dist", "shape", "point"),
        "records": ("q", "B") + (("d_max", "shape_bits") if cloud else GRASP + ("d_max",)) + ("per_shape", "dist", "shape", "point", "witness", "jrows"),
        "distances": ("q", "B") + GRASP + ("out_d",),
        "item_records": ("q", "B") + GRASP + ("dist", "witness", "jrows"),
        "listed_records": ("q", "B", "items", "N") + GRASP + ("dist", "witness", "jrows"),
        "edges": ("starts", "goals", "dist", "E", "resolution", "max_distance", "mode", "threshold") + SEL[family] +
                 ("accumulate", "valid", "end", "n_samples", "workspace", "workspace_bytes"),
        "splines": ("ctrl", "S", "n_ctrl", "degree", "knots", "resolution", "threshold") + SEL[family] +
                   ("accumulate", "valid", "t_hit", "n_samples", "workspace", "workspace_bytes"),
        "edges_ca": ("starts", "goals", "dist", "E", "max_distance", "mode", "threshold", "max_iter", "slack") + look + SEL[family] +
                    ("accumulate", "valid", "end", "t_free", "status"),
        "splines_ca": ("ctrl", "S", "n_ctrl", "degree", "knots", "threshold", "max_iter", "slack") + look + SEL[family] +
                      ("accumulate", "valid", "t_free", "status"),
    }[kind]
    return HEAD[family] + body + ("stream",)


# entry -> (family, kind, the workspace-size export of a sampled entry)
ENTRIES = {
    "nbk_cloud_validity_batch": ("cloud", "validity", None),
    "nbk_cloud_clearance_batch": ("cloud", "clearance", None),
    "nbk_records_cloud_batch": ("cloud", "records", None),
    "nbk_edge_cloud_validity_batch": ("cloud", "edges", "nbk_edge_cloud_workspace_bytes"),
    "nbk_spline_cloud_validity_batch": ("cloud", "splines", "nbk_spline_cloud_workspace_bytes"),
    "nbk_edge_cloud_continuous_batch": ("cloud", "edges_ca", None),
    "nbk_spline_cloud_continuous_batch": ("cloud", "splines_ca", None),
    "nbk_held_validity_batch": ("held", "validity", None),
    "nbk_held_distances_batch": ("held", "distances", None),
    "nbk_held_records_batch": ("held", "item_records", None),
    "nbk_held_records_items": ("held", "listed_records", None),
    "nbk_edge_held_validity_batch": ("held", "edges", "nbk_edge_held_workspace_bytes"),
    "nbk_spline_held_validity_batch": ("held", "splines", "nbk_spline_held_workspace_bytes"),
    "nbk_edge_held_continuous_batch": ("held", "edges_ca", None),
    "nbk_spline_held_continuous_batch": ("held", "splines_ca", None),
    "nbk_held_cloud_validity_batch": ("held_cloud", "validity", None),
    "nbk_held_cloud_clearance_batch": ("held_cloud", "clearance", None),
    "nbk_held_cloud_records_batch": ("held_cloud", "records", None),
    "nbk_edge_held_cloud_validity_batch": ("held_cloud", "edges", "nbk_edge_held_cloud_workspace_bytes"),
    "nbk_spline_held_cloud_validity_batch": ("held_cloud", "splines", "nbk_spline_held_cloud_workspace_bytes"),
    "nbk_edge_held_cloud_continuous_batch": ("held_cloud", "edges_ca", None),
    "nbk_spline_held_cloud_continuous_batch": ("held_cloud", "splines_ca", None),
}
ROW_KINDS = ("validity", "clearance", "records", "distances", "item_records", "listed_records")
COUNT = {"edges": "E", "edges_ca": "E", "splines": "S", "splines_ca": "S"}
# the arrays a kind needs when there is something to do, and the outputs it may be asked for besides
NEEDED = {"validity": ("q",), "clearance": ("q", "min_dist"), "records": ("q", "dist"), "distances": ("q",), "item_records": ("q", "dist"),
          "listed_records": ("q", "items", "dist"), "edges": ("starts", "goals", "valid", "workspace"),
          "splines": ("ctrl", "knots", "valid", "workspace"), "edges_ca": ("starts", "goals", "valid", "t_free", "status"),
          "splines_ca": ("ctrl", "knots", "valid", "t_free", "status")}
ARRAYS = ("q", "min_dist", "dist", "out_d", "items", "starts", "goals", "valid", "workspace", "ctrl", "knots", "t_free", "status", "mask_bytes")


class Buffers:
    """The stand-ins of one test (kept alive by it)."""

    def __init__(self):
        self._m = (C.c_char * 4096)()
        C.memset(self._m, 0x7f, 4096)
        self._held = (C.c_char * 4096)()
        self._mem = np.zeros((1 << 16,), dtype=np.uint8)
        self.m, self.held = C.addressof(self._m), C.addressof(self._held)
        self.base = self._mem.ctypes.data + (-self._mem.ctypes.data) % 64


def _good(lib, buf, entry, n=4):
    """-> arguments of ``entry`` that pass every rule of its own, for n rows / edges / trajectories"""
    family, kind, ws = ENTRIES[entry]
    a = dict.fromkeys(_order(family, kind))
    a.update(m=buf.m, held=buf.held, c=buf.m)
    a.update({k: buf.base for k in ARRAYS if k in a})
    a.update({k: v for k, v in dict(B=n, E=n, S=n, N=n, grasp_rows=0, threshold=0.0, accumulate=0, d_max=0.3, per_shape=0, resolution=0.05,
                                    max_distance=0.25, mode=0, n_ctrl=6, degree=3, max_iter=50, slack=1e-3, look_ahead=0.1).items() if k in a})
    if ws is not None:
        a["workspace_bytes"] = getattr(lib, ws)(max(n, 0))
    return a


def _call(lib, buf, entry, n=4, **kw):
    a = _good(lib, buf, entry, n)
    a.update(kw)
    family, kind, _ = ENTRIES[entry]
    return getattr(lib, entry)(*[a[k] for k in _order(family, kind)])


def _past(entry):
    """what an entry answers once its own rules are through: it asks whose the handles are"""
    return (INVALID, DEVICE if ENTRIES[entry][0] == "cloud" else FOREIGN)


def _nothing(entry):
    """what it answers to n == 0: the sampled and certified entries and nbk_records_cloud_batch before the handles are looked at,
    every other row entry behind them"""
    return (OK, None) if ENTRIES[entry][1] not in ROW_KINDS or entry == "nbk_records_cloud_batch" else _past(entry)


def _cases(lib, buf, entry):
    """-> [(what, n or None, arguments that differ from the good ones, code, text or None)]"""
    family, kind, ws = ENTRIES[entry]
    names = _order(family, kind)
    rows = kind in ROW_KINDS
    count = "N" if kind == "listed_records" else ("B" if rows else COUNT[kind])
    bad = lambda what, **kw: (what, None, kw, INVALID, None)                                  # noqa: E731
    out = [("every rule passes", None, {}, *_past(entry))]
    # ---- single faults
    out += [bad(f"null {h}", **{h: None}) for h in HEAD[family]]
    out += [bad(f"negative {count}", **{count: -1})] + [bad(f"null {k}", **{k: None}) for k in NEEDED[kind]]
    if kind == "listed_records":
        out += [bad("negative B", B=-1)]
    if kind == "validity":
        # (the cloud's own verdict entry has no threshold rule: a NaN threshold is the kernel's to answer)
        out += [bad("no mask", mask_bytes=None), ("the packed mask alone", None, dict(mask_bits=buf.base, mask_bytes=None), *_past(entry)),
                ("NaN threshold", None, dict(threshold=nan), *(_past(entry) if family == "cloud" else (INVALID, None))),
                ("nothing to do and a NaN threshold", 0, dict(threshold=nan), *(_past(entry) if family == "cloud" else (INVALID, None)))]
    if "d_max" in names:
        out += [bad(f"d_max {v}", d_max=v) for v in (nan, inf, -inf)]
    if "grasp_rows" in names:
        out += [bad("grasp_rows 7", grasp=buf.base, grasp_rows=7), bad("grasp_rows -1", grasp=buf.base, grasp_rows=-1),
                bad("rows without a grasp", grasp_rows=1), bad("a row each without a grasp", grasp_rows=4), bad("a grasp without rows", grasp=buf.base),
                ("one grasp row", None, dict(grasp=buf.base, grasp_rows=1), *_past(entry)),
                ("a grasp row each", None, dict(grasp=buf.base, grasp_rows=4), *_past(entry))]
    if "max_distance" in names:
        out += [bad("max_distance 0", max_distance=0.0), bad("max_distance NaN", max_distance=nan), bad("mode 2", mode=2), bad("mode -1", mode=-1)]
    if "degree" in names:
        out += [bad("degree 0", degree=0), bad("degree 6", degree=6, n_ctrl=8), bad("n_ctrl equal to the degree", n_ctrl=3),
                bad("n_ctrl 65537", n_ctrl=65537)]
    if "resolution" in names:
        out += [bad(f"resolution {v}", resolution=v) for v in (0.0, -0.05, nan)] + [bad("NaN threshold", threshold=nan)]
        out += [bad("workspace one byte short", workspace_bytes=getattr(lib, ws)(4) - 1), bad("workspace of no bytes", workspace_bytes=0),
                bad("workspace off by 8 bytes", workspace=buf.base + 8, workspace_bytes=1 << 15),
                bad("workspace off by 32 bytes", workspace=buf.base + 32, workspace_bytes=1 << 15)]
        if kind == "splines":
            out += [bad("resolution inf", resolution=inf)]
    if "max_iter" in names:
        out += [bad("max_iter 0", max_iter=0), bad("negative slack", slack=-1e-3), bad("NaN slack", slack=nan), bad("NaN threshold", threshold=nan)]
    if "look_ahead" in names:
        out += [bad(f"look_ahead {v}", look_ahead=v) for v in (0.0, -1.0, nan)] + [("look_ahead inf", None, dict(look_ahead=inf), *_past(entry))]
    if "grasp" in names and not rows:
        out += [("the call's grasp", None, dict(grasp=buf.base), *_past(entry))]
    if family == "cloud":
        # a selection on a descriptor of more than 256 robot shapes: refused where the handles are looked at, before the device
        out += [("a selection on too many shapes", None, dict(shape_bits=buf.base), UNSUPPORTED, None)]
    # ---- nothing to do
    nulls = {k: None for k in names if k in ARRAYS or k in ("end", "n_samples", "t_hit", "shape", "point", "witness", "jrows", "mask_bits")}
    zero = dict(nulls, workspace_bytes=0) if ws else nulls
    out += [("nothing to do", 0, {}, *_nothing(entry)), ("nothing to do, null outputs", 0, zero, *_nothing(entry)),
            ("nothing to do, null handles", 0, dict(zero, **{h: None for h in HEAD[family]}), INVALID, None)]
    if kind == "listed_records":
        out += [("no rows and a list", None, dict(B=0, q=None), *_past(entry)), bad("no rows, no list and a negative B", N=0, B=-1)]
    if kind in ("distances", "item_records"):
        out += [("no rows", 0, dict(q=None), *_past(entry))]
    # ---- the size limits
    if kind == "splines":
        out += [("2**26 trajectories", 2**26, dict(workspace_bytes=0), UNSUPPORTED, None),
                ("2**26 - 1 trajectories, no workspace bytes", 2**26 - 1, dict(workspace_bytes=0), INVALID, None)]
    if kind == "edges":
        out += [("edges above EDGE_CLOUD_MAX_E", 2**56 + 1, dict(workspace_bytes=0), UNSUPPORTED, None),
                ("2**31 edges and their workspace", 2**31, {}, UNSUPPORTED, None),
                ("2**31 edges, no workspace bytes", 2**31, dict(workspace_bytes=0), INVALID, None)]
    if kind in ("edges_ca", "splines_ca"):
        out += [("2**31 trajectories", 2**31, {}, UNSUPPORTED, None), ("2**31 - 1 trajectories", 2**31 - 1, {}, *_past(entry))]
    # ---- two faults at once: the order decides
    if not rows:
        out += [("nothing to do and a NaN threshold", 0, dict(threshold=nan), INVALID, None),
                ("nothing to do and a null handle", 0, {HEAD[family][-1]: None}, INVALID, None),
                ("too many and a NaN threshold", 2**56 + 1, dict(threshold=nan, workspace_bytes=0) if ws else dict(threshold=nan), INVALID, None),
                ("too many and a null output", 2**56 + 1, dict(valid=None), INVALID, None)]
    if ws:
        out += [("short workspace and a NaN threshold", None, dict(workspace_bytes=0, threshold=nan), INVALID, None),
                ("nothing to do and a misaligned workspace", 0, dict(workspace=buf.base + 8), OK, None)]
    if "grasp_rows" in names:
        # (the held object is the foreign one in every case: a grasp fault is answered first, and leaves no text)
        out += [("bad grasp rows and a foreign held object", None, dict(grasp=buf.base, grasp_rows=7), INVALID, None),
                ("bad grasp rows, nothing to do", 0, dict(grasp=buf.base, grasp_rows=7), INVALID, None),
                ("a grasp without rows, nothing to do", 0, dict(grasp=buf.base), *_past(entry)),
                ("nothing to do and a foreign held object", 0, {}, *_past(entry))]
    if "look_ahead" in names:
        out += [("nothing to do and look_ahead 0", 0, dict(look_ahead=0.0), INVALID, None)]
    return out


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_entry_rules(entry):
    lib = _lib.load()
    buf = Buffers()
    sentinel_entry = "nbk_cloud_validity_batch" if ENTRIES[entry][0] != "cloud" else "nbk_held_validity_batch"
    sentinel = _past(sentinel_entry)[1]
    seen = set()
    for what, n, kw, code, text in _cases(lib, buf, entry):
        assert what not in seen, f"{entry}: two cases named {what!r}"
        seen.add(what)
        assert _call(lib, buf, sentinel_entry) == INVALID and lib.nbk_last_error().decode().startswith(sentinel)
        got = _call(lib, buf, entry, **({} if n is None else {"n": n}), **kw)
        err = lib.nbk_last_error().decode()
        assert got == code, f"{entry}, {what}: returned {got}, expected {code} ({err!r})"
        assert err.startswith(sentinel if text is None else text), f"{entry}, {what}: left {err!r}, expected {text!r}"


def test_the_table_holds_every_entry_of_the_three_families():
    lib = _lib.load()
    for entry, (family, kind, ws) in ENTRIES.items():
        assert entry in _lib.SYMBOLS and hasattr(lib, entry), entry
        assert len(getattr(lib, entry).argtypes) == len(_order(family, kind)), entry
        assert ws is None or ws in _lib.SYMBOLS
    batch = [s for s in _lib.SYMBOLS if ("cloud" in s or "held" in s) and (s.endswith("_batch") or s == "nbk_held_records_items") and
             not s.startswith("nbk_frame_")]
    assert sorted(batch) == sorted(ENTRIES), "an entry of the three families is missing from the table"
