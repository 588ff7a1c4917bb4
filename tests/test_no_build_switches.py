"""The kernel sources carry one code path per kernel: no `#ifndef X / #define X default` build switch, no `#if` arm that the
product never builds.  An experiment may add a switch while it runs; what is committed has decided it.  Every preprocessor
conditional under csrc/ must test a symbol of the short list below - compiler or target predicates, and the one
instrumentation hook named there.  The assembly generators (csrc/gen_*.py) read no environment and no command line: a
variant that ships is an argument of generate(), and what a generator prints is the same under any environment."""
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "opencv-simpleslam_amd" / "csrc"

ALLOWED = {
    # compiler / target predicates
    "__HIP_DEVICE_COMPILE__", "__has_builtin", "__has_include", "__has_attribute", "__gfx950__", "__cplusplus",
    # not an A/B: the per-phase clock stamps of the fused FFN, read by scripts/ubench/ffn_fused_bench.hip.  Its store target is a
    # member of FfnFusedArgs in the middle of the kernel arguments, so it cannot leave without moving the default build's code.
    "FFN_STAMP",
}
CONDITIONAL = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif)\b(.*)$")
IDENT = re.compile(r"[A-Za-z_]\w*")


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def test_csrc_has_no_experiment_switches():
    sources = sorted(CSRC.glob("*.hip")) + sorted(CSRC.glob("*.hpp"))
    assert sources, f"no kernel sources under {CSRC}"
    bad = []
    for src in sources:
        for no, line in enumerate(_strip_comments(src.read_text()).splitlines(), 1):
            m = CONDITIONAL.match(line)
            if not m:
                continue
            names = set(IDENT.findall(m.group(2))) - {"defined"}
            if not names or names - ALLOWED:
                bad.append(f"{src.name}:{no}: {line.strip()}")
    assert not bad, ("build switches in the kernel sources - decide the A/B, then delete the loser:\n  " + "\n  ".join(bad))


def test_the_scan_sees_every_conditional_form():
    text = _strip_comments("#ifndef X\n  # if defined(Y) && __has_builtin(z)\n#elif 1\n// #if COMMENTED\n#ifdef FFN_STAMP\n#else\n#endif\n")
    hits = [CONDITIONAL.match(l) for l in text.splitlines()]
    assert [bool(h) for h in hits] == [True, True, True, False, True, False, False]


# ---- the assembly generators (csrc/gen_*.py) follow the same rule: a generator's text is a function of its file alone
ENV_READ = re.compile(r"os\.environ|getenv|sys\.argv|runpy")
GENERATORS = sorted(CSRC.glob("gen_*.py"))
# every switch the attention generator once read, at a value that changed its text then
RETIRED = {"ATTN_ASM_ABL": "novalu", "ATTN_ASM_PK": "1", "ATTN_ASM_STAMP": "1", "ATTN_ASM_DEFER": "1", "ATTN_ASM_NEXP_ODD": "2",
           "ATTN_ASM_DMA_FIRST": "4", "ATTN_ASM_WEIGHTED": "1", "ATTN_ASM_P1": "1", "ATTN_ASM_KERNEL": "x"}


def _run_generator(gen, extra_env):
    """the text a generator prints, run the way build.py runs it (python <absolute path>), here from another directory"""
    clean = {k: val for k, val in os.environ.items() if k not in RETIRED}
    res = subprocess.run([sys.executable, str(gen)], capture_output=True, text=True, env={**clean, **extra_env}, cwd=str(ROOT / "tests"))
    assert res.returncode == 0, f"{gen.name} failed:\n{res.stderr}"
    return res.stdout


@pytest.fixture(scope="module")
def generated():
    assert [g.name for g in GENERATORS] == ["gen_lg_attention_asm.py", "gen_lg_attention_asm_p1.py"]
    return {g.stem: _run_generator(g, {}) for g in GENERATORS}


def test_generators_read_no_environment():
    assert GENERATORS, f"no generators under {CSRC}"
    bad = [f"{g.name}:{no}: {line.strip()}" for g in GENERATORS
           for no, line in enumerate(g.read_text().splitlines(), 1) if ENV_READ.search(line)]
    assert not bad, "a generator's text must depend on its file alone - make the variant an argument:\n  " + "\n  ".join(bad)


def test_the_scan_sees_every_environment_read():
    lines = ["X = os.environ.get('A', '0')", "os.environ['A'] = '1'", "from os import getenv", "y = os.getenv('A')",
             "if len(sys.argv) > 1:", "import runpy", "runpy.run_path(p)",
             "import sys", "sys.stdout.write(generate(False))", "environment = 1", "import os.path"]
    assert [bool(ENV_READ.search(l)) for l in lines] == [True] * 7 + [False] * 4


def test_generator_output_ignores_the_environment(generated):
    for g in GENERATORS:
        assert _run_generator(g, RETIRED) == generated[g.stem], f"{g.name} prints another text with the retired switches set"


def test_each_generator_declares_its_own_kernel(generated):
    base, p1 = generated["gen_lg_attention_asm"], generated["gen_lg_attention_asm_p1"]
    def declared(text):
        return set(re.findall(r"^\s*\.amdhsa_kernel\s+(\w+)\s*$", text, re.M)) | set(re.findall(r"^\s*\.globl\s+(\w+)\s*$", text, re.M))
    assert declared(base) == {"lg_attention_asm_kernel"} and "lg_attention_asm_p1_kernel" not in base
    assert declared(p1) == {"lg_attention_asm_p1_kernel"}
    assert base != p1
    for text in (base, p1):
        assert re.findall(r"^\s*\.amdhsa_kernarg_size\s+(\d+)\s*$", text, re.M) == ["128"]
