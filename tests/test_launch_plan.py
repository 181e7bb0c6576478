"""The planning CU count and the launch log (csrc/hip/launch_plan.hip) are test hooks: nothing in the package sets
them, no environment variable reaches them, and both are inert by default. (Their effect on the kernel forms is
tested on the GPU: test_gpu_launch_forms.py.)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_import_never_sets_planning_override():
    """A fresh interpreter that imports the package, its runtime front-end and the native module has no override,
    whatever CU-count-looking variables the environment holds."""
    env = dict(os.environ, DASH_PLANNING_CUS="1", DASH_NUM_CUS="1", DASH_CUS="1", HIP_PLANNING_CUS="1")
    code = ("import dash_amd, dash_amd.runtime, dash_amd.serving\n"
            "from dash_amd.native import native\n"
            "n = native()\n"
            "print('override', n.hip_planning_override(), len(n.hip_launch_log_take()))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[-3:] == ["override", "0", "0"], r.stdout


def test_planning_state_has_no_environment_knob():
    src = open(os.path.join(ROOT, "dash_amd", "csrc", "hip", "launch_plan.hip")).read()
    assert "getenv" not in src and "environ[" not in src


def test_set_and_restore(native):
    base = native.hip_planning_cus()  # without a device: the planning default
    assert base >= 1 and native.hip_planning_override() == 0
    native.hip_set_planning_cus(3)
    try:
        assert native.hip_planning_cus() == 3 and native.hip_planning_override() == 3
    finally:
        native.hip_set_planning_cus(0)
    assert native.hip_planning_cus() == base and native.hip_planning_override() == 0
