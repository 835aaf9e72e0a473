"""km_live_device_bytes counts what the library holds on the device: 0 after load, and a create that fails for want of a
device holds nothing and hands nothing out.  Runs in a child process of its own with every GPU hidden, so it sees a freshly
loaded library and the same failure on a machine with a GPU as on one without."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import ctypes as C
from koemorph_amd import _lib
lib = _lib.load()
assert lib.km_live_device_bytes() == 0, lib.km_live_device_bytes()
SENTINEL = 0x5A5A5A50
for name, args in (("km_attn_stats_create", (28, 80, 0)), ("km_metrics_create", ())):
    out = C.c_void_p(SENTINEL)
    rc = getattr(lib, name)(C.byref(out), *args)
    assert rc == _lib.KM_ERR_HIP, (name, rc, lib.km_last_error())
    assert out.value == SENTINEL, (name, out.value)
    assert lib.km_live_device_bytes() == 0, (name, lib.km_live_device_bytes())
print("ok")
"""


def test_counter_is_zero_after_load_and_a_failed_create_holds_nothing():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    res = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stdout + res.stderr
