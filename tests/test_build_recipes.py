"""The two recipes of the HIP library -- ndtpso_slam_amd/build.py and host/CMakeLists.txt -- compile the same translation units
with the same flags: both read csrc/hip_units.txt and csrc/hip_flags.txt.  (A unit that reached one compile line only once
left the CMake build unable to link.)  Nothing is compiled here."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ndtpso_slam_amd", "csrc")
# the flags that are part of the numerical contract (ndtpso_slam_amd/build.py says why)
CONTRACT = ["-O3", "-ffp-contract=off", "-fno-fast-math", "-mllvm", "-enable-ipra=0", "--offload-arch=gfx950", "-std=c++17"]


def _hip_units():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))


def _cmake_compile_line():
    """The hipcc COMMAND of host/CMakeLists.txt with its file(STRINGS ...) lists read the way CMake reads them."""
    text = open(os.path.join(ROOT, "host", "CMakeLists.txt")).read()
    text = re.sub(r"(?m)#.*$", "", text)
    values = {"NDTPSO_CSRC": CSRC}
    for path, var in re.findall(r"file\(STRINGS\s+(\S+)\s+(\w+)\)", text):
        path = path.replace("${NDTPSO_CSRC}", CSRC)
        values[var] = [line.strip() for line in open(path) if line.strip()]
    for var, prefix in re.findall(r"list\(TRANSFORM\s+(\w+)\s+PREPEND\s+(\S+)\)", text):
        values[var] = [prefix.replace("${NDTPSO_CSRC}", CSRC) + v for v in values[var]]
    command = re.search(r"COMMAND\s+\$\{NDTPSO_HIPCC\}(.*?)\n\s*DEPENDS", text, re.S).group(1)
    line = []
    for word in command.split():
        m = re.fullmatch(r"\$\{(\w+)\}", word)
        if m and isinstance(values.get(m.group(1)), list):
            line += values[m.group(1)]
        else:
            line.append(word.replace("${NDTPSO_CSRC}", CSRC))
    return line


def _is_sublist(needle, hay):
    return any(hay[i:i + len(needle)] == needle for i in range(len(hay)))


def test_both_recipes_compile_every_unit_with_the_contract_flags():
    from ndtpso_slam_amd import build
    units = _hip_units()
    assert len(units) >= 3
    lines = {"build.py": build.FLAGS + build.SRCS, "CMakeLists.txt": _cmake_compile_line()}
    for name, line in lines.items():
        on_line = sorted(os.path.basename(w) for w in line if w.endswith(".hip"))
        assert on_line == units, (name, on_line)
        for w in line:
            if w.endswith(".hip"):
                assert os.path.samefile(os.path.dirname(w), CSRC), (name, w)
        for flag in CONTRACT:
            assert flag in line, (name, flag)
        assert _is_sublist(["-mllvm", "-enable-ipra=0"], line), name
    # the two lines differ by build.py's warning flags and by nothing else
    flags = {name: [w for w in line if not w.endswith(".hip") and w not in ("-o", "${NDTPSO_HIP_LIB}")] for name, line in lines.items()}
    assert [f for f in flags["build.py"] if not f.startswith("-W")] == flags["CMakeLists.txt"]
    units_in_order = {name: [os.path.basename(w) for w in line if w.endswith(".hip")] for name, line in lines.items()}
    assert units_in_order["build.py"] == units_in_order["CMakeLists.txt"]


def test_a_build_depends_on_every_source_file():
    from ndtpso_slam_amd import build
    deps = {os.path.realpath(d) for d in build.DEPS}
    for f in os.listdir(CSRC):
        assert os.path.realpath(os.path.join(CSRC, f)) in deps, f
    assert os.path.realpath(os.path.join(ROOT, "include", "ndtpso_hip.h")) in deps
    cmake = open(os.path.join(ROOT, "host", "CMakeLists.txt")).read()
    assert re.search(r"file\(GLOB\s+NDTPSO_HIP_DEPS\s+CONFIGURE_DEPENDS\s+\$\{NDTPSO_CSRC\}/\*\)", cmake)
    assert re.search(r"DEPENDS\s+\$\{NDTPSO_HIP_DEPS\}\s+\$\{NDTPSO_ROOT\}/include/ndtpso_hip\.h", cmake)
