"""CPU: the conditions that make tests/test_gpu_stream_delay.py's comparisons meaningful, on the
oracle alone (tests/delay_ref.py holds the runs), and the ABI of the per-stream delay.

1. The margin rule of tests/test_gpu_batch_kv8.py: (top1 - top2) / max|logit| >= 4 x the logit
   bar on every step of every stream of every run, none left out, for the exact (delay, frames,
   seed) triples the GPU tests replay.
2. A wrong ada table must be visible: a stream's steps decoded with a neighbouring delay's table
   move the logits by at least 100 x the bar.
3. The new entry points are declared in both headers and bound in the Python mirror with matching
   signatures.
"""
import ctypes
import os
import re

import pytest

import delay_ref as d
from conftest import ROOT

pytestmark = pytest.mark.cpu


@pytest.mark.parametrize("name", ["single", "f32", "kv16", "q8"])
def test_margin_rule_on_every_step_of_every_stream(name):
    rule = d.MARGIN_KV16 if d.RUNS[name][3] else d.MARGIN_F32
    ref = d.oracle(name, only=(0, 3)) if name == "single" else d.oracle(name)
    d.assert_margin(ref, rule, f"stream delay run {name}")
    if name != "single":
        # every delay is there, and every stream takes at least the six steps whose logits are read
        assert {d.delay_of(i) for i in range(len(ref))} == set(d.DELAYS)
        assert min(len(ids) for ids, _ in ref) >= 6
        for i, (ids, _) in enumerate(ref):
            assert len(ids) == d.frames(i) // 8 - (32 + d.delay_of(i)), i


@pytest.mark.parametrize("cfg", ["TINY", "KV8"])
@pytest.mark.parametrize("delay,wrong", [(12, 6), (12, 11), (3, 1)])
def test_wrong_table_is_visible(cfg, delay, wrong):
    """measured on the CPU oracle: 5e-2 to 3e-1 of the largest logit"""
    shift = d.wrong_table_shift(cfg, delay, wrong)
    print(f"{cfg}: delay {delay} decoded with the table of {wrong}: logits move by {shift:.2e} of the largest")
    assert shift >= 100 * d.LOGIT_TOL, (cfg, delay, wrong, shift)


def _declared(header, prefix):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(2): (m.group(1).strip(), [a.strip() for a in m.group(3).split(",")])
            for m in re.finditer(r"^([a-z_ ]+?)\s*\*?\b(%s[a-z0-9_]+)\s*\(([^)]*)\)\s*;" % prefix, src, flags=re.M)}


def _ctype(arg):
    if "*" in arg:
        return ctypes.POINTER(ctypes.c_float) if arg.startswith("float") else ctypes.c_void_p
    return ctypes.c_int


def test_abi_of_the_stream_delay_entry_points():
    import vox_hip
    dec = _declared("voxtral_hip.h", "vox_hip_")
    want = {"vox_hip_stream_set_delay": ("int", ["vox_hip_stream_t *s", "int delay_tokens"]),
            "vox_hip_stream_delay": ("int", ["const vox_hip_stream_t *s"]),
            "vox_hip_stream_ada_scale": ("int", ["vox_hip_stream_t *s", "float *out"])}
    lib = ctypes.CDLL(vox_hip.LIB_PATH)
    for name, sig in want.items():
        assert dec.get(name) == sig, (name, dec.get(name))
        assert hasattr(lib, name), name
        assert name in vox_hip.EXPORTS, name
    hdr = open(os.path.join(ROOT, "include", "voxtral_hip.h")).read()
    assert re.search(r"#define\s+VOX_HIP_MAX_DELAY_TOKENS\s+30\b", hdr)
    assert vox_hip.MAX_DELAY_TOKENS == 30
    hdec = _declared("vox_hip_host.h", "vh_")
    hwant = {"vh_stream_set_delay": ("int", ["vh_stream_t *s", "int delay_ms"]),
             "vh_stream_delay_ms": ("int", ["const vh_stream_t *s"])}
    hlib = ctypes.CDLL(os.path.join(ROOT, "voxtral.c_amd", "libvox_hip_host.so"))
    for name, sig in hwant.items():
        assert hdec.get(name) == sig, (name, hdec.get(name))
        assert hasattr(hlib, name), name
    # the Python mirror binds them with the declared argument and result types (the libraries
    # load without a GPU; nothing is called)
    L, H = vox_hip.lib(), vox_hip.host_lib()
    for lib_, table in ((L, want), (H, hwant)):
        for name, (res, args) in table.items():
            fn = getattr(lib_, name)
            assert fn.restype is ctypes.c_int and res == "int", name
            assert list(fn.argtypes) == [_ctype(a) for a in args], (name, fn.argtypes)
    for cls, names in ((vox_hip.Stream, ("set_delay", "delay_tokens", "ada_scale")),
                       (vox_hip.HostStream, ("set_delay", "delay_ms"))):
        for n in names:
            assert hasattr(cls, n), (cls.__name__, n)
