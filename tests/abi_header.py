"""What the CPU tests read out of include/*.h and out of the compiled device code: the declared entry points, struct fields and
#define constants of a header, and the private-segment (scratch) size of every kernel of a csrc file."""
import ctypes
import importlib.util
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
# signature letter -> ctypes type, restated here so that what _lib.bind set is checked against the header and not against _lib
CTYPES = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_int64, "f": ctypes.c_float, "d": ctypes.c_double}
RETURNS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p}


def read_header(name):
    """The text of include/<name> without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, name)).read(), flags=re.S)


def parse_header(name):
    """-> {entry point: (return type, argument signature)} with the letters of _lib.SIGNATURES."""
    decls = {}
    for m in re.finditer(r"\b(int64_t|int|const char\*)\s+(micf_\w+)\s*\(([^)]*)\)\s*;", read_header(name)):
        sig = ""
        for a in [a.strip() for a in m.group(3).split(",") if a.strip() and a.strip() != "void"]:
            if "*" in a or a.startswith("micf_stream_t"):
                sig += "p"
            elif a.startswith("int64_t"):
                sig += "l"
            elif a.startswith("int "):
                sig += "i"
            elif a.startswith("float "):
                sig += "f"
            elif a.startswith("double "):
                sig += "d"
            else:
                raise AssertionError(f"unparsed argument {a!r} in {m.group(2)}")
        decls[m.group(2)] = (m.group(1), sig)
    return decls


def struct_decls(name, struct):
    """The member declarations of `typedef struct NAME { ... } NAME;` in order, e.g. ["void* out", "int32_t out_shape[3]"]."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), read_header(name), re.S).group(1)
    return [d.strip() for d in body.split(";") if d.strip()]


def struct_fields(name, struct):
    """The member names in declaration order; "const float *a, *b" declares two."""
    return [part.replace("*", " ").split()[-1] for decl in struct_decls(name, struct) for part in decl.split(",")]


def defines(name, prefix):
    """-> {macro: value} of the integer `#define <prefix>...` lines."""
    return {k: int(v) for k, v in re.findall(r"#define (%s\w+) (\d+)" % prefix, read_header(name))}


def build_module():
    """micformer_amd/build.py loaded by path (it needs no built library)."""
    spec = importlib.util.spec_from_file_location("_micformer_build", os.path.join(ROOT, "micformer_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    return build


def device_asm(source):
    """Compiles csrc/<source> to device assembly with the project's flags.
    -> ({kernel: private-segment bytes}, the assembly, the flags)."""
    build = build_module()
    assert source in build.SOURCES
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, os.path.splitext(source)[0] + ".s")
        r = subprocess.run([build._hipcc()] + flags + ["-S", "--cuda-device-only", os.path.join(build.CSRC, source), "-o", out],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        asm = open(out).read()
    sizes = re.findall(r"\.amdhsa_kernel\s+(\S+).*?\.amdhsa_private_segment_fixed_size\s+(\d+)", asm, flags=re.S)
    assert len(sizes) == len(set(k for k, _ in sizes)) == asm.count(".amdhsa_private_segment_fixed_size")
    return {k: int(v) for k, v in sizes}, asm, flags
