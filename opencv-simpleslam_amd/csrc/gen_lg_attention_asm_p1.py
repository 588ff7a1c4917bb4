#!/usr/bin/env python3
"""The attention kernel of the opt-in precision "f16x3p1" (P as one fp16 plane in P.V; sslam_lightglue_set_precision(lg, 2)):
generate(True) of gen_lg_attention_asm.py, as a code object of its own (lg_attention_asm_p1_kernel)."""
import sys

from gen_lg_attention_asm import generate      # the sibling: a script's own directory is sys.path[0]

sys.stdout.write(generate(True))
