#!/usr/bin/env python3
"""Are the device functions of two builds of libmrirt.so the same code?  The check a move-only refactor of csrc/ is held to.

Both libraries are disassembled (device_disassembly of tools/check_async_loads.py) and split by symbol.  Every symbol must
exist in both with the same instruction sequence once what depends on WHERE the function was linked is taken out: the
`// address: encoding <target>` comment, and the literals of the s_add_u32 / s_addc_u32 pair that follows an s_getpc_b64
(PC-relative addresses; branch operands are relative already).  Every kernel must also have the same register, LDS and
scratch figures in its code object's metadata note (llvm-readelf --notes).  Exit status 0 = identical.

    python3 tools/compare_code_objects.py <before/libmrirt.so> <after/libmrirt.so>
"""
import pathlib
import re
import subprocess
import sys
import tempfile

from check_async_loads import ADDR, code_objects, device_disassembly, llvm_bin

FIGURES = ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
           "private_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size", "uses_dynamic_stack")


def functions(so):
    """{symbol: [instruction text]} of every device function of the library"""
    funcs, cur, pcrel = {}, None, 0
    for line in device_disassembly(so).splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        ins = line.split("//")[0].strip()
        if cur is None or not ins or not ADDR.search(line):     # (an instruction line carries its address and encoding)
            continue
        if pcrel and re.match(r"s_addc?_u32\b", ins):
            ins = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "<pcrel>", ins)
        pcrel = 4 if ins.startswith("s_getpc_b64") else max(pcrel - 1, 0)
        cur.append(ins)
    return funcs


def figures(so):
    """{kernel: {figure: value}} from the metadata notes of the library's code objects"""
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for co in code_objects(so, pathlib.Path(td)):
            notes = subprocess.run([str(llvm_bin() / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True, check=True).stdout
            for block in re.split(r"\n  - (?=\.)", notes)[1:]:                    # one entry of amdhsa.kernels
                kv = dict(re.findall(r"^    \.(\w+):\s+(\S+)$", block, re.M) + re.findall(r"^\.(\w+):\s+(\S+)$", block, re.M))
                out[kv["name"]] = {k: kv.get(k) for k in FIGURES}
    return out


def main():
    a, b = (pathlib.Path(p) for p in sys.argv[1:3])
    fa, fb, ga, gb = functions(a), functions(b), figures(a), figures(b)
    bad = 0
    for name in sorted(set(fa) ^ set(fb)):
        bad += 1
        print(f"ONLY IN {'BEFORE' if name in fa else 'AFTER'}: {name}")
    for name in sorted(set(ga) ^ set(gb)):
        bad += 1
        print(f"KERNEL ONLY IN {'BEFORE' if name in ga else 'AFTER'}: {name}")
    for name in sorted(set(fa) & set(fb)):
        if fa[name] != fb[name]:
            bad += 1
            first = next((i for i, (x, y) in enumerate(zip(fa[name], fb[name])) if x != y), min(len(fa[name]), len(fb[name])))
            print(f"CODE DIFFERS {name}: {len(fa[name])} vs {len(fb[name])} instructions, first difference at #{first}:")
            print(f"   before: {fa[name][first] if first < len(fa[name]) else '(end)'}\n   after:  {fb[name][first] if first < len(fb[name]) else '(end)'}")
    for name in sorted(set(ga) & set(gb)):
        if ga[name] != gb[name]:
            bad += 1
            print(f"FIGURES DIFFER {name}: " + ", ".join(f"{k} {ga[name][k]} -> {gb[name][k]}" for k in FIGURES if ga[name][k] != gb[name][k]))
    n = sum(len(v) for v in fb.values())
    print(f"compare_code_objects: {len(fb)} device functions ({len(gb)} kernels, {n} instructions): " + ("identical" if not bad else f"{bad} difference(s)"))
    return 1 if bad or not fb or not gb else 0


if __name__ == "__main__":
    sys.exit(main())
