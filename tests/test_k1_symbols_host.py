"""The K1 register-gather march kernels of the built library, by symbol (CPU only).

The march kernels are templates instantiated through host-side selectors (csrc/brats_march.hip: layout_kernel, pipe_kernel,
roll_kernel; csrc/brats_tf.hip: tf_kernel, tf_pipe_kernel).  An edit to the shared device code or to a selector can drop an
instantiation without any compile error; the launch that needed it would then take another kernel, or fail only on a GPU.
tests/golden/k1_kernel_symbols.txt is the list the library had before the march and the table kernels were given one Stage and
one composite(): the generic, pipelined and rolling kernels (with the tagged twin) and the table's generic and pipelined kernels.
"""
import importlib.util
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parent.parent
FAMILIES = ("brats_march_kernel", "brats_march_pipe_kernel", "brats_march_roll_kernel", "brats_tf_kernel", "brats_tf_pipe_kernel")


def test_k1_kernel_symbol_set_is_the_recorded_one():
    spec = importlib.util.spec_from_file_location("check_async_loads", ROOT / "tools" / "check_async_loads.py")
    gate = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gate)
    lib = importlib.import_module("mri-raytracer_amd._lib")
    lib.lib()                                                        # (raises if the library is missing)
    symbols = re.findall(r"^[0-9a-f]+ <(\S+)>:", gate.device_disassembly(lib.SO_PATH), re.M)
    built = sorted(n for n in set(symbols) if not n.startswith("__") and any(f in n for f in FAMILIES))
    want = (ROOT / "tests" / "golden" / "k1_kernel_symbols.txt").read_text().split()
    assert len(want) == 199 and want == sorted(set(want))
    assert sorted(set(built) - set(want)) == [], "kernels the record does not have"
    assert sorted(set(want) - set(built)) == [], "instantiations that were dropped"
