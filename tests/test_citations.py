"""Every `file:line` citation of the reference in the oracle, the public headers, the kernels and the host shim points at lines
that exist.  The judge checks parity through these citations; a citation that has drifted past the end of its file, or names a
file the reference does not have, is caught here.  For the two shader files the whole path rests on, a few anchor identifiers are
also checked at the cited lines.  What the reference holds comes from tests/golden/reference_citations.json (its files' line
counts, and the lines of a few anchor identifiers; tools/make_fixtures.py reference_citations), which is checked against the
reference itself where that is mounted."""
import json
import os
import re

import pytest

from conftest import GOLDEN, REFERENCE, ROOT

FIXTURE = json.load(open(os.path.join(GOLDEN, "reference_citations.json")))
HAVE_REFERENCE = os.path.isdir(os.path.join(REFERENCE, "src"))

CITING = ["oracle/bb_oracle.c", "oracle/bb_oracle.h", "oracle/scenes.py", "include/bibim_hip.h", "include/bibim_scene.h",
          "include/bibim_assets.h", "bibim_renderer_amd/csrc/bb_kernels.hip.h", "bibim_renderer_amd/csrc/bb_types.h",
          "bibim_renderer_amd/csrc/bb_scene.cpp", "bibim_renderer_amd/csrc/bb_assets.cpp", "bibim_renderer_amd/csrc/bibim_hip.hip",
          "INTEGRATION.md", "DESIGN.md"]
CITE = re.compile(r"((?:src/)?(?:[\w]+/)*[\w]+\.(?:frag|vert|geom|glsl|cpp|h|inl|bff|toml)):(\d+)(?:-(\d+))?(?:,\s*(\d+)(?:-(\d+))?)*")


def _reference_files():
    """basename -> [(path relative to the reference's root, line count)]"""
    out = {}
    for rel, n in FIXTURE["line_counts"].items():
        out.setdefault(os.path.basename(rel), []).append((rel, n))
    return out


@pytest.mark.skipif(not HAVE_REFERENCE, reason="the reference is not mounted here: the committed fixture stands for it")
def test_fixture_is_the_reference_where_it_is_mounted():
    suffixes = (".frag", ".vert", ".geom", ".glsl", ".cpp", ".h", ".inl", ".bff", ".toml")
    counts = {}
    for base, _dirs, files in os.walk(REFERENCE):
        if os.sep + "external" in base:
            continue
        for f in files:
            if f.endswith(suffixes):
                counts[os.path.relpath(os.path.join(base, f), REFERENCE)] = sum(1 for _ in open(os.path.join(base, f), errors="replace"))
    assert counts == FIXTURE["line_counts"]
    for name, tokens in FIXTURE["anchors"].items():
        lines = open(os.path.join(REFERENCE, "src", "shaders", name), errors="replace").read().splitlines()
        assert tokens == {t: [i + 1 for i, l in enumerate(lines) if t in l] for t in tokens}, name


def test_cited_lines_exist():
    files = _reference_files()
    own = {os.path.basename(p) for p in CITING} | {"bb_oracle.c", "bench.py"}
    checked = 0
    for rel in CITING:
        text = open(os.path.join(ROOT, rel)).read()
        for m in CITE.finditer(text):
            name = m.group(1)
            base = os.path.basename(name)
            if base in own or base not in files:     # the repository's own files (bench.py:343) or third-party headers not cited by line
                assert base in own or not name.startswith("src/"), f"{rel} cites {name}, which the reference does not have"
                continue
            cands = [(p, n) for p, n in files[base] if p.endswith(name)] or files[base]
            n_lines = max(n for _, n in cands)
            last = max(int(g) for g in re.findall(r"\d+", m.group(0).split(":", 1)[1]))
            assert last <= n_lines, f"{rel} cites {m.group(0)} but {base} has {n_lines} lines"
            checked += 1
    assert checked > 150, checked      # (the oracle and the headers cite the reference line by line)


def test_anchor_identifiers_stand_where_the_oracle_says():
    brdf, frag, vert = "brdf.glsl", "forward_brdf.frag", "forward_brdf.vert"
    for name, a, b, tokens in ((brdf, 2, 36, ("distributionGGX", "geometrySchlickGGX", "geometrySmith", "fresnelSchlick", "pow(")),
                               (brdf, 4, 15, ("NdotH2", "a2 - 1", "PI * denom * denom")),
                               (frag, 15, 76, ("uNumLights", "innerCutOff", "0.001", "vec3(0.03)", "outColor")),
                               (frag, 29, 70, ("light.type == 0", "light.type == 2", "normalize(L + V)", "kD *= (1 - metallic)")),
                               (vert, 24, 37, ("aModel", "uProjMat", "uViewMat", "aInvModel", "cross("))):
        for t in tokens:
            assert any(a <= line <= b for line in FIXTURE["anchors"][name][t]), f"{name}:{a}-{b} no longer holds `{t}`"
