"""Host resources own themselves (csrc/bb_own.h): the owners' behaviour where every acquisition fails -- a stand-alone program
under the address and UB sanitizers, run with an empty device list, so the same here and on a GPU machine -- and the source
rule that keeps it so: nothing in csrc/bibim_hip.hip frees, unpins or destroys by hand."""
import os
import re
import shutil
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "bibim_renderer_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH") or "/opt/rocm"
RELEASES = {"hipFree(": "DeviceBuffer", "hipHostFree(": "PinnedBlock", "hipEventDestroy(": "Event", "hipStreamDestroy(": "Stream"}


def test_owners_under_address_and_ub_sanitizers_without_a_device(tmp_path):
    """tests/own_check.cpp with the host compiler against the HIP runtime, the sanitizers' runtimes linked into the program"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "own_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(ROCM, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "own_check.cpp"),
                           "-o", exe, "-L" + os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib")])
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")      # no device: the program never opens a GPU
    p = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count(" ok\n") == 5 and "WRONG" not in p.stdout, p.stdout


def _bodies(text, opening):
    """{name: body} of the top-level blocks whose first line matches `opening` (one group: the name) and which end at the next
    line that starts with a closing brace"""
    out = {}
    for m in re.finditer(opening, text, flags=re.M):
        end = re.compile(r"^\}", re.M).search(text, m.end())
        out[m.group(1)] = text[m.start():end.end()]
    return out


def test_nothing_is_released_by_hand():
    hip = open(os.path.join(CSRC, "bibim_hip.hip")).read()
    free = _bodies(hip, r"^int (bbr_device_free)\(")["bbr_device_free"]       # the caller's memory: not the library's to own
    assert free.count("hipFree(") == 1 and len(free.splitlines()) < 12
    rest = hip.replace(free, "")
    for call in RELEASES:
        assert call not in rest, f"bibim_hip.hip calls {call}...) outside bbr_device_free: hold the resource in an owner (bb_own.h)"
    own = open(os.path.join(CSRC, "bb_own.h")).read()
    owners = _bodies(own, r"^struct (\w+) \{")
    assert set(RELEASES.values()) <= set(owners)
    for call, owner in RELEASES.items():
        assert owners[owner].count(call) == 1 and own.count(call) == 1, f"{call}...) belongs in {owner}::release() and nowhere else"
    # the header stands alone: a program without the kernels or the context includes it (tests/own_check.cpp)
    assert re.findall(r'#include "([^"]+)"', own) == []
