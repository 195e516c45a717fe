"""Register / LDS / scratch usage of the device kernels in libazsp.so (reads the gfx950 code object out of the fat binary with
llvm-readelf --notes).  usage: python tools/kernel_resources.py [substring of the kernel name]"""
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def code_object(lib):
    data = open(lib, "rb").read()
    i = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    n = struct.unpack_from("<Q", data, i + 24)[0]
    off = i + 32
    for _ in range(n):
        o, sz, tl = struct.unpack_from("<QQQ", data, off)
        off += 24
        trip = data[off:off + tl].decode()
        off += tl
        if "gfx950" in trip:
            return data[i + o:i + o + sz]
    raise SystemExit("no gfx950 code object in " + lib)


def resources(co_path):
    """{demangled kernel name: (vgpr+agpr, agpr, sgpr, lds bytes, scratch bytes)} of a code object file"""
    notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", co_path], capture_output=True, text=True, check=True).stdout
    names = subprocess.run(["c++filt"], input="\n".join(re.findall(r"\.name:\s+(\S+)", notes)), capture_output=True,
                           text=True).stdout.split("\n")
    out = {}
    for k, blk in enumerate(notes.split("- .agpr_count:")[1:]):
        g = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
        out[names[k] if k < len(names) else "?"] = (g("vgpr_count"), int(blk.split()[0]), g("sgpr_count"), g("group_segment_fixed_size"),
                                                    g("private_segment_fixed_size"))
    return out


def main():
    pat = sys.argv[1] if len(sys.argv) > 1 else ""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(code_object(os.path.join(ROOT, "alpha_zero_amd", "libazsp.so")))
        f.flush()
        res = resources(f.name)
    for name, (vgpr, agpr, sgpr, lds, scratch) in res.items():
        if pat in name:
            print(f"{name[:110]:110s} vgpr+agpr {vgpr:3d} (agpr {agpr:3d}) sgpr {sgpr:3d} lds {lds:6d} scratch {scratch}")


if __name__ == "__main__":
    main()
