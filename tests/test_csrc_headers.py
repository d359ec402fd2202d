"""CPU-side checks of csrc/ as a set of files: every header compiles when it is the only one included (device side, syntax only), and
the source hash that decides whether a built library is stale covers every file the library is compiled from.  No GPU."""
import os
import re
import subprocess

import pytest

from reachy2_symbolic_ik_amd import build

CSRC = build.CSRC
# Not headers that stand alone, by design (each says so in its first lines):
FRAGMENTS = {
    "rsik_poly_gen.hpp": "generated; included in the middle of rsik_math.hpp, inside namespace rsik",
    "rsik_cont_run.hpp": "host code included inside rsik_lib.hip's extern \"C\" block, uses its statics",
    "rsik_comm.hpp": "host code included inside rsik_lib.hip's extern \"C\" block, uses its statics",
}
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".hpp") and f not in FRAGMENTS)
INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', re.M)


def hipcc_or_skip():
    try:
        return build.hipcc()
    except RuntimeError as e:
        pytest.skip(str(e))


def test_the_fragments_exist_and_say_what_they_are():
    for name in FRAGMENTS:
        with open(os.path.join(CSRC, name)) as fh:
            head = "".join(fh.readline() for _ in range(3))
        assert "fragment by design" in head, name


@pytest.mark.parametrize("header", HEADERS)
def test_every_header_compiles_alone(header, tmp_path):
    hipcc = hipcc_or_skip()
    src = tmp_path / "only.hip"
    src.write_text(f'#include "{header}"\n')
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-fsyntax-only", "-I", CSRC, str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{header} does not compile on its own:\n{r.stderr[-4000:]}"


def test_source_hash_covers_every_included_file():
    deps = {os.path.normpath(os.path.join(CSRC, d)) for d in build.DEPS}
    for d in deps:
        assert os.path.isfile(d), f"build.DEPS names {d}, which does not exist"
    reached, todo = set(), [os.path.normpath(os.path.join(CSRC, s)) for s in build.SOURCES]
    while todo:
        path = todo.pop()
        if path in reached:
            continue
        reached.add(path)
        with open(path) as fh:
            for inc in INCLUDE.findall(fh.read()):
                todo.append(os.path.normpath(os.path.join(os.path.dirname(path), inc)))
    assert len(reached) > len(HEADERS), "the walk found no includes"
    assert reached <= deps, f"compiled into the library but not in build.DEPS (the source hash): {sorted(reached - deps)}"
