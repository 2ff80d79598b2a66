"""The host side of the SAM batch path (hsa_amd.sam.device_sam): the string layout, the
binding's struct against the C header, and the call without a device.  No GPU needed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unpack(data, off):
    return [data[int(off[k]):int(off[k + 1])].tobytes() for k in range(len(off) - 1)]


def test_pack_strings_round_trips():
    from hsa_amd.sam import pack_strings
    items = ["", "r", "x" * 255, "", "read/1", "", b"\x21\x7e"]
    data, off = pack_strings(items)
    assert data.dtype == np.uint8 and off.dtype == np.uint64 and len(off) == len(items) + 1
    assert int(off[0]) == 0 and int(off[-1]) == len(data) == 1 + 255 + 6 + 2
    assert (np.diff(off.astype(np.int64)) >= 0).all()
    assert unpack(data, off) == [x.encode() if isinstance(x, str) else x for x in items]
    data, off = pack_strings([])
    assert len(data) == 0 and off.tolist() == [0]
    data, off = pack_strings(["", ""])
    assert len(data) == 0 and off.tolist() == [0, 0, 0]
    data, off = pack_strings(["q"])
    assert data.tolist() == [ord("q")] and off.tolist() == [0, 1]


def test_line_bound_covers_the_longest_fields():
    """Every number at its type's most digits, every string at its stated length."""
    from hsa_amd import sam
    from hsa_amd._lib import HSA_SAM_MAX_LINE
    big = 2 ** 64 - 1
    line = "\t".join(["n" * 7, str(2 ** 32 - 1), "c" * 5, str(big), str(2 ** 32 - 1), "268435455M" * 4, "*", "0", "0",
                      "A" * 50, "I" * 50, "XT:A:U", f"NM:i:{2 ** 32 - 1}", f"X0:i:{big}", f"X1:i:{big}", "XM:i:65535",
                      "XO:i:255", "XG:i:510", "MD:Z:" + "0" * 20,
                      "XA:Z:" + ("c" * 5 + f",+{big}" + "268435455M" * 4) * 2 + "c" * 5 + f",-{big},66045;"]) + "\n"
    assert len(line) <= sam.line_bound(7, 50, 5, 4, 20, 3)
    assert len(line) > sam.line_bound(7, 50, 5, 4, 20, 2)                  # (and not by a wide margin)
    assert sam.line_bound(255, 60000, 5, 4, 20, 3) == HSA_SAM_MAX_LINE


def test_sam_batch_struct_matches_the_header(tmp_path):
    """sizeof and every offsetof of hsa_sam_batch64_t, from a C program compiled against
    include/hsa_gpu.h."""
    from hsa_amd._lib import SamBatch64
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    fields = [f[0] for f in SamBatch64._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "hsa_gpu.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(hsa_sam_batch64_t));\n'
                   + "".join(f'    printf("{f} %zu\\n", offsetof(hsa_sam_batch64_t, {f}));\n' for f in fields)
                   + "    return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == C.sizeof(SamBatch64)
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out[1:] if ln}
    assert got == {f: getattr(SamBatch64, f).offset for f in fields}
    assert len(got) == 35


def test_sam_lines_without_a_device_fail_loudly():
    """No handle can exist without a GPU, so the call answers for itself: HSA_E_NODEV
    where no device is visible (HSA_E_ARG for the missing handle where one is)."""
    from hsa_amd import _lib
    gi = _lib.GpuIndex.__new__(_lib.GpuIndex)
    code = -3 if _lib.device_count() < 1 else -2
    with pytest.raises(_lib.HsaError, match=f"error {code}:"):
        gi.sam_lines64(_lib.SamBatch64())
    assert b"hsa_sam_lines_device64" in _lib.lib().hsa_last_error()
