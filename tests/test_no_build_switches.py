"""The kernel sources carry one code path per kernel: no `#ifndef X / #define X default` build switch, no `#if` arm that the
product never builds.  An experiment may add a switch while it runs; what is committed has decided it.  Every preprocessor
conditional under csrc/ must test a symbol of the short list below - compiler or target predicates, and the one
instrumentation hook named there."""
import re
from pathlib import Path

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
