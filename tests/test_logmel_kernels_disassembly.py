"""Static guard for DESIGN.md section 2b (no GPU needed), with the mechanics of tests/test_packed_fp32_forms.py: every
kernel of the library whose name contains `logmel` -- producers, which the pipeline runs on the background stream beside
the sweeps -- holds no packed-fp32 instruction, and the kernels of the even sizes that are not powers of two (mixed
radix and Bluestein) are among them."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "audio_tokens_amd" / "libaudio_tokens_amd.so"
OBJDUMP = Path("/opt/rocm/lib/llvm/bin/llvm-objdump")


@pytest.fixture(scope="module")
def logmel_kernels(tmp_path_factory):
    if not LIB.exists() or not OBJDUMP.exists():
        pytest.skip("needs the built library and ROCm's llvm-objdump")
    work = tmp_path_factory.mktemp("codeobj")
    shutil.copy(LIB, work / LIB.name)
    subprocess.run([str(OBJDUMP), "--offloading", LIB.name], cwd=work, check=True, capture_output=True)
    objs = sorted(work.glob("*gfx950*"))
    assert objs, "no gfx950 code object found in the library"
    out = {}
    for o in objs:
        dis = subprocess.run([str(OBJDUMP), "-d", str(o)], check=True, capture_output=True, text=True).stdout
        name = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                name = m.group(1) if "logmel" in m.group(1) else None
                if name:
                    out.setdefault(name, [])
            elif name is not None and "v_pk_" in line:
                out[name].append(line.split("//")[0].strip())
    return out


def test_new_kernels_are_in_the_library(logmel_kernels):
    mixed = [n for n in logmel_kernels if "logmel_mixed_kernel" in n]
    # form 1 (mixed radix, BLUE = false) and form 2 (Bluestein), each over the uniform and the plan clip map
    assert len(mixed) == 4 and sum("ILb0E" in n for n in mixed) == 2 and sum("ILb1E" in n for n in mixed) == 2, mixed
    assert any("logmel_any_kernel" in n for n in logmel_kernels) and any("logmel_kernel" in n for n in logmel_kernels)


def test_no_logmel_kernel_holds_a_packed_fp32_instruction(logmel_kernels):
    for n, ins in logmel_kernels.items():
        assert not ins, f"{n}: {len(ins)} packed-fp32 instructions, e.g. {ins[0]}"
