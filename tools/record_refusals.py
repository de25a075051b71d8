#!/usr/bin/env python
"""Record what the DG entry points answer to calls they refuse before any device work:

    FEINSUM_HIP_LIB=<parent>/libfeinsum_hip.so python tools/record_refusals.py [tests/golden/refusals.json]

Every entry point -- the named ones, fe_launch with every family and modifier bit, fe_launch_f32 -- is driven with a call
that has one fault of each class of the argument check's precedence ("the front end"), and with every pair of
classes.  The table holds the entry point, the case and the return code, no messages.  tests/test_refusals_cpu.py replays
it against the built library.  Pointers are small integers: nothing here may reach a device, so a case that a library does
not refuse (a return code other than FE_EINVAL / FE_EUNSUPPORTED, or FE_OK without E = 0) is not recorded."""
from __future__ import annotations

import ctypes
import itertools
import json
import math
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from feinsum_amd import _hip   # noqa: E402

GRAD, DIV, GRADDIV, FACEMASS, DIVCOMP, MATAPPLY = 1, 2, 3, 4, 5, 7
F32, ACC, FIELDS_F32 = _hip.FAMILY_F32, _hip.FAMILY_ACC, _hip.FAMILY_FIELDS_F32

#: the fault classes, in the order of the precedence: name -> (class of the precedence, the knobs it sets)
FAULTS = {
    "none": (0, {}),   # the call as it stands, where that is refused already
    # 1. structure
    "E<0": (1, {"E": -1}),
    "Np<=0": (1, {"Np": 0}),
    "nf<=0": (1, {"nf": 0}),
    "b<1": (1, {"b": 0}),
    "flags": (1, {"flags": 8}),
    "alpha": (1, {"alpha": math.nan}),
    "beta": (1, {"beta": math.inf}),
    "null table": (1, {"tables": False}),
    "null pack": (1, {"pack": False}),
    "ld<E": (1, {"ld_short": True}),
    "ld large": (1, {"ld": 1 << 40}),
    "J misaligned": (1, {"J": 12}),
    "field misaligned": (1, {"fld": 10}),
    "output misaligned": (1, {"out": 12}),
    # 2. scope
    "Np=56": (2, {"Np": 56}),
    "Nfp": (2, {"Nfp": 14}),
    "b=1": (2, {"b": 1}),
    "variant": (2, {"variant": 99}),
    # 3. nothing to do
    "E=0": (3, {"E": 0}),
    # 4. null pointers, sizes beyond the index arithmetic
    "J null": (4, {"J": 0}),
    "operator null": (4, {"op": 0}),
    "field null": (4, {"fld": 0}),
    "E*Np": (4, {"E": 1 << 35, "ld": 1 << 36}),
}

BASE = dict(J=8, op=8, fld=8, out=8, E=10, Np=35, nf=4, Nfp=15, b=2, flags=0, variant=0, alpha=0.5, beta=2.0, ld=20,
            ld_short=False, tables=True, pack=True)

_COMMON = ["E<0", "Np<=0", "flags", "J misaligned", "field misaligned", "output misaligned", "E=0", "J null", "operator null",
           "field null", "E*Np"]
_TABLES = ["b<1", "null table"]
_FACES = ["nf<=0", "Nfp", "b=1"]
_AB = ["alpha", "beta"]
_LD = ["ld<E", "ld large"]


def _tables(k):
    if not k["tables"]:
        return None, None
    n = max(k["b"], 1)
    return _hip._ptr_array([k["fld"]] * n), _hip._ptr_array([k["out"]] * n)


def _pack(k):
    pack = _hip.ArgPack()
    pack.J, pack.D, pack.u, pack.out, pack.v_div, pack.out2 = k["J"], k["op"], k["fld"], k["out"], k["fld"], k["out"]
    v, o = _tables(k)
    if v is not None:
        pack.v, pack.outs = v, o
    pack.E, pack.Np, pack.nf, pack.Nfp, pack.b, pack.ndim = k["E"], k["Np"], k["nf"], k["Nfp"], k["b"], 3
    pack.layout_flags, pack.variant, pack.alpha, pack.beta = k["flags"], k["variant"], k["alpha"], k["beta"]
    return pack, (v, o)


def _named(name, order):
    def call(lib, k):
        v, o = _tables(k)
        ld = k["E"] - 1 if k["ld_short"] else k["ld"]
        n = max(k["b"], 1)
        j3 = _hip._ptr_array([k["J"]] * 3)                                          # the three geometry-factor planes
        o3 = _hip._ptr_array([k["out"]] * (3 * n)) if k["tables"] else None         # three output planes per field
        values = dict(k, v=v, o=o, u=k["fld"], ld=ld, none=None, j3=j3, o3=o3, two=2)
        return getattr(lib, name)(*[values[key] for key in order.split()])
    return call


def _launch(entry, family):
    def call(lib, k):
        pack, keep = _pack(k)
        return getattr(lib, entry)(family, ctypes.byref(pack) if k["pack"] else None, None)
    return call


#: entry point -> (how to call it, what its messages start with, the fault classes that apply to it)
ENTRIES = {
    "fe_grad3d_prepared_f64": (_named("fe_grad3d_prepared_f64", "J op none v o E Np b flags variant none"), ("grad:",),
                               _COMMON + _TABLES + ["variant"]),
    "fe_div3d_prepared_f64": (_named("fe_div3d_prepared_f64", "J op none v o E Np b flags variant none"), ("div:",),
                              _COMMON + _TABLES + ["variant"]),
    "fe_divcomp3d_f64": (_named("fe_divcomp3d_f64", "J op u out E Np flags variant none"), ("div component:",), _COMMON + ["variant"]),
    "fe_matapply_f64": (_named("fe_matapply_f64", "J op v o E Np b flags variant none"), ("matapply:",),
                        [f for f in _COMMON if f != "J null"] + _TABLES + ["variant"]),
    "fe_graddiv3d_prepared_f64": (_named("fe_graddiv3d_prepared_f64", "J op none u u out out E Np variant none"),
                                  ("graddiv:", "grad:", "div:"), [f for f in _COMMON if f != "flags"] + ["variant"]),
    "fe_gradplanes3d_f64": (_named("fe_gradplanes3d_f64", "j3 op v o3 E Np b flags variant none"), ("grad planes:", "div component:"),
                            _COMMON + _TABLES + ["variant"]),
    # ndim = 2: the triangle paths of the n-dimensional entry points
    "fe_grad_f64(ndim=2)": (_named("fe_grad_f64", "J op v o E two Np b flags variant none"), ("grad:",), _COMMON + _TABLES + ["variant"]),
    "fe_div_f64(ndim=2)": (_named("fe_div_f64", "J op v o E two Np b flags variant none"), ("div:",), _COMMON + _TABLES + ["variant"]),
    "fe_divcomp_f64(ndim=2)": (_named("fe_divcomp_f64", "J op u out E two Np flags variant none"), ("div component:",),
                               _COMMON + ["variant"]),
    "fe_waveop3d_prepared_f64": (_named("fe_waveop3d_prepared_f64", "J op none u out u out J op none v o E Np nf Nfp b flags variant none"),
                                 ("waveop:", "graddiv:", "grad:", "div:", "face-mass"), [f for f in _COMMON if f != "flags"] + ["variant"]),
    # (a fused call; what the fused launch does not serve goes to the graddiv and face-mass entry points)
    "fe_waveop3d_f64": (_named("fe_waveop3d_f64", "J op u out u out J op v o E Np nf Nfp b flags variant none"),
                        ("waveop:", "graddiv:", "grad:", "div:", "face-mass"), [f for f in _COMMON if f != "flags"] + ["variant"]),
    "fe_facemass_prepared_f64": (_named("fe_facemass_prepared_f64", "J op none v o E Np nf Nfp b flags variant none"), ("face-mass",),
                                 _COMMON + _TABLES + ["nf<=0", "variant"]),
    "fe_facemass_acc_f64": (_named("fe_facemass_acc_f64", "J op v o E Np nf Nfp b flags alpha beta none"), ("accumulating face-mass:",),
                            _COMMON + _TABLES + _FACES + _AB + ["Np=56"]),
    "fe_grad3d_acc_f64": (_named("fe_grad3d_acc_f64", "J op u out E Np flags alpha beta none"), ("accumulating grad:",),
                          _COMMON + _AB + ["Np=56"]),
    "fe_div3d_acc_f64": (_named("fe_div3d_acc_f64", "J op u out E Np flags alpha beta none"), ("accumulating div:",),
                         _COMMON + _AB + ["Np=56"]),
    "fe_grad3d_strided_f64": (_named("fe_grad3d_strided_f64", "J ld op v o ld E Np b flags none"), ("grad on an element slice:",),
                              _COMMON + _TABLES + _LD + ["Np=56"]),
    "fe_div3d_strided_f64": (_named("fe_div3d_strided_f64", "J ld op v ld o E Np b flags none"), ("div on an element slice:",),
                             _COMMON + _TABLES + _LD + ["Np=56"]),
    "fe_facemass_strided_f64": (_named("fe_facemass_strided_f64", "J ld op v ld o E Np nf Nfp b flags none"),
                                ("face-mass on an element slice:",), _COMMON + _TABLES + _FACES + _LD + ["Np=56"]),
    "fe_grad3d_mixed_f64": (_named("fe_grad3d_mixed_f64", "J op v o E Np b flags none"), ("grad, float32 fields:",),
                            _COMMON + _TABLES + ["Np=56"]),
    "fe_div3d_mixed_f64": (_named("fe_div3d_mixed_f64", "J op v o E Np b flags none"), ("div, float32 fields:",),
                           _COMMON + _TABLES + ["Np=56"]),
    "fe_facemass_mixed_f64": (_named("fe_facemass_mixed_f64", "J op v o E Np nf Nfp b flags none"), ("face-mass, float32 fields:",),
                              _COMMON + _TABLES + ["nf<=0", "Nfp", "Np=56"]),
}
_PACK = ["null pack"]
_LAUNCHES = {   # family -> (message prefixes besides "fe_launch", fault classes)
    GRAD: (("grad:",), _COMMON + ["variant"]),
    DIV: (("div:",), _COMMON + ["variant"]),
    GRADDIV: (("graddiv:", "grad:", "div:"), [f for f in _COMMON if f != "flags"] + ["variant"]),
    FACEMASS: (("face-mass",), _COMMON + _TABLES + ["nf<=0", "variant"]),
    DIVCOMP: (("div component:",), _COMMON + ["variant"]),
    MATAPPLY: (("matapply:",), [f for f in _COMMON if f != "J null"] + _TABLES + ["variant"]),
    ACC | GRAD: (("accumulating grad:",), _COMMON + _AB + ["Np=56", "null table"]),
    ACC | DIV: (("accumulating div:",), _COMMON + _AB + ["Np=56", "null table"]),
    ACC | FACEMASS: (("accumulating face-mass:",), _COMMON + _TABLES + _FACES + _AB + ["Np=56"]),
    FIELDS_F32 | GRAD: (("grad, float32 fields:",), _COMMON + ["Np=56"]),
    FIELDS_F32 | DIV: (("div, float32 fields:",), _COMMON + ["Np=56"]),
    FIELDS_F32 | FACEMASS: (("face-mass, float32 fields:",), _COMMON + ["nf<=0", "Nfp", "Np=56"]),
    F32 | GRAD: (("fe_launch_f32:",), ["E<0", "Np<=0", "flags", "E=0", "J null", "operator null", "field null"]),
    F32 | DIV: (("fe_launch_f32:",), ["E<0", "Np<=0", "flags", "E=0", "J null", "operator null", "field null"]),
    F32 | FACEMASS: (("fe_launch_f32:",), ["E<0", "Np<=0", "nf<=0", "E=0", "J null", "operator null", "field null"]),
    F32 | DIVCOMP: (("fe_launch_f32:",), ["E<0", "Np<=0", "flags", "E=0", "J null", "operator null", "field null"]),
    F32 | MATAPPLY: (("fe_launch_f32:",), ["E<0", "Np<=0", "flags", "E=0", "operator null", "field null"]),
    F32 | GRADDIV: (("fe_launch_f32:",), ["none", "E<0", "Np<=0", "E=0"]),     # no float32 kernel: the plain call is refused
    ACC | MATAPPLY: ((), []),              # no such kernel: refused by fe_launch itself
    FIELDS_F32 | MATAPPLY: ((), []),
    FIELDS_F32 | ACC | GRAD: ((), []),
    99: ((), []),
}
for _family, (_who, _faults) in _LAUNCHES.items():
    ENTRIES[f"fe_launch(0x{_family:x})"] = (_launch("fe_launch", _family), ("fe_launch:",) + _who, _faults + _PACK)
for _family in (GRAD, DIV, FACEMASS, DIVCOMP, MATAPPLY, GRADDIV):
    _who, _faults = _LAUNCHES[F32 | _family]
    ENTRIES[f"fe_launch_f32(0x{_family:x})"] = (_launch("fe_launch_f32", _family), _who, _faults + _PACK)


def cases(entry):
    """(case name, knobs) of an entry point: each fault alone, then each pair of two faults that set different knobs"""
    faults = ENTRIES[entry][2]
    for name in faults:
        yield name, dict(BASE, **FAULTS[name][1])
    for a, b in itertools.combinations(faults, 2):
        ka, kb = FAULTS[a][1], FAULTS[b][1]
        if set(ka) & set(kb):
            continue
        yield f"{a} + {b}", dict(BASE, **ka, **kb)
    if not faults:
        yield "plain", dict(BASE)


def refused(rc, knobs):
    return rc in (_hip.FE_EINVAL, _hip.FE_EUNSUPPORTED) or (rc == _hip.FE_OK and knobs["E"] == 0)


def run(lib, entry, knobs):
    call = ENTRIES[entry][0]
    rc = call(lib, knobs)
    return rc, lib.fe_last_error() or b""


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tests" / "golden" / "refusals.json"
    os.environ.setdefault("HIP_VISIBLE_DEVICES", "-1")   # (nothing here needs a device, and nothing may reach one)
    lib = _hip.load_library()
    table, dropped = [], []
    for entry in ENTRIES:
        for case, knobs in cases(entry):
            rc, _ = run(lib, entry, knobs)
            (table if refused(rc, knobs) else dropped).append({"entry": entry, "case": case, "rc": rc})
    by_entry = {}   # entry point -> case -> return code
    for row in table:
        by_entry.setdefault(row["entry"], {})[row["case"]] = row["rc"]
    out.write_text(json.dumps({"library": "the parent commit's", "cases": by_entry}, indent=0, separators=(",", ":")) + "\n")
    print(f"{len(table)} refusals of {len(ENTRIES)} entry points recorded in {out}")
    for d in dropped:
        print("not refused before device work, not recorded:", d)


if __name__ == "__main__":
    main()
