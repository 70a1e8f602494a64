"""Register, scratch and LDS footprint of the frame's kernels, read from the compiler's own device listing.

k_geometry's waves wait for memory most of their lives, and with frames in flight they share their SIMDs with k_raster's and
k_shade's: what they hold of the register file, not what they compute, is what they cost the pipelined frame.  All kernels
live in one header, so the test also pins that the neighbours did not grow.

gfx950 hands out vector registers in steps of 8 from 512 per SIMD lane: an allocation of 128 / 96 / 80 / 72 / 64 registers
lets 4 / 5 / 6 / 7 / 8 waves share a SIMD as far as the vector file goes.

No GPU is needed: the library's source is compiled for gfx950 with the flags of bibim_renderer_amd/csrc/Makefile (taken from
`make -n`, so they cannot drift apart) up to the device assembly, whose metadata carries the numbers."""
import os
import re
import shlex
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bibim_renderer_amd", "csrc")

GEOMETRY_LDS_MAX = 3520         # one ClipWork per wave, as before the kernel was reordered
GEOMETRY_VGPR_HARD_MAX = 96     # 5 waves per SIMD: strictly more than the 4 of the 112-register kernel this one replaces
GEOMETRY_VGPR_SHIPPED_MAX = 64  # the step of 8 waves per SIMD, the footprint of k_raster and k_shade: what the kernel ships with
RASTER_VGPR_MAX = 64
# plain k_shade<32, 32, DEFERRED, PRESENT, TAIL = false, MIXED = false>
SHADE_VGPR_MAX = {(0, 0): 58, (0, 1): 58, (1, 0): 60, (1, 1): 60}
ANISO_VGPR_MAX = 128            # the allocation step of the four waves per SIMD k_shade_aniso runs at


def _makefile_command():
    """the hipcc command line the Makefile would run, as a list of words"""
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC], check=True, capture_output=True, text=True).stdout
    lines = [l for l in out.splitlines() if "bibim_hip.hip" in l and "hipcc" in l]
    assert len(lines) == 1, out
    return shlex.split(lines[0])


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    words = _makefile_command()
    hipcc = words[0]
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc on this machine")
    flags, skip_next = [], False
    for w in words[1:]:
        if skip_next:
            skip_next = False
        elif w == "-o":
            skip_next = True
        elif w in ("-shared", "-lz") or w.endswith((".hip", ".cpp")):
            pass
        else:
            flags.append(w)
    listing = str(tmp_path_factory.mktemp("isa") / "bibim_hip.s")
    cmd = [hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(CSRC, "bibim_hip.hip"), "-o", listing]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    text = open(listing).read()
    meta = text[text.index("amdhsa.kernels:"):]
    found = {}
    for block in re.split(r"\n  - (?=\.agpr_count:)", meta)[1:]:
        def field(key):
            return re.search(r"\n?\s*\." + key + r":\s*(\S+)", block).group(1)
        found[field("name")] = {k: int(field(k)) for k in
                                ("vgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    assert found, "no kernel metadata in the device listing"
    return found


def _one(kernels, prefix):
    names = [n for n in kernels if n.startswith(prefix)]
    assert len(names) == 1, (prefix, names)
    return kernels[names[0]]


@pytest.mark.parametrize("tile", [32, 64])
def test_k_geometry_footprint(kernels, tile):
    k = _one(kernels, f"_ZN3bbr10k_geometryILi{tile}ELi{tile}ELb0EEE")
    print(f"k_geometry<{tile},{tile},false>: {k}")
    assert k["private_segment_fixed_size"] == 0, "k_geometry owns scratch"
    assert k["group_segment_fixed_size"] <= GEOMETRY_LDS_MAX
    assert k["agpr_count"] == 0
    assert k["vgpr_count"] <= GEOMETRY_VGPR_HARD_MAX      # at least 5 waves per SIMD
    assert k["vgpr_count"] <= GEOMETRY_VGPR_SHIPPED_MAX   # the allocation step of 8 waves per SIMD


def test_k_raster_did_not_grow(kernels):
    k = _one(kernels, "_ZN3bbr8k_rasterILi32ELi32ELb0EEE")
    print(f"k_raster<32,32,false>: {k}")
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_count"] <= RASTER_VGPR_MAX


@pytest.mark.parametrize("deferred,present", sorted(SHADE_VGPR_MAX))
def test_k_shade_did_not_grow(kernels, deferred, present):
    k = _one(kernels, f"_ZN3bbr7k_shadeILi32ELi32ELb{deferred}ELb{present}ELb0ELb0EEE")
    print(f"k_shade<32,32,{deferred},{present},false,false>: {k}")
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_count"] <= SHADE_VGPR_MAX[(deferred, present)]


@pytest.mark.parametrize("deferred,present", sorted(SHADE_VGPR_MAX))
def test_k_shade_aniso_stays_at_four_waves(kernels, deferred, present):
    k = _one(kernels, f"_ZN3bbr13k_shade_anisoILi32ELi32ELb{deferred}ELb{present}ELb0EEE")
    print(f"k_shade_aniso<32,32,{deferred},{present},false>: {k}")
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_count"] <= ANISO_VGPR_MAX
