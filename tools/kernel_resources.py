"""Per-kernel resource listing (VGPR / AGPR / SGPR / scratch / LDS / occupancy) of HIP sources, from hipcc's
-Rpass-analysis=kernel-resource-usage remarks; needs no GPU.  One line per kernel symbol, sorted, so two listings diff cleanly:

    python tools/kernel_resources.py conv_igemm_bf16.hip dwconv_bf16.hip > after.txt
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from multitask_bonetumor_yolo_amd import build as B  # noqa: E402

FIELDS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def listing(src):
    cmd = [B.HIPCC] + B.FLAGS + B.EXTRA_FLAGS.get(src, []) + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                                              os.path.join(B.CSRC, src), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    rows, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*(.+?): (\S+))\s*\[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1):
            cur = rows.setdefault(m.group(1), {})
        elif cur is not None and m.group(2) in FIELDS:
            cur[m.group(2)] = m.group(3)
    return [f"{src} {name} " +  " ".join(f"{k.split(' [')[0].replace(' ', '')}={v.get(k, '?')}" for k in FIELDS) for name, v in sorted(rows.items())]


if __name__ == "__main__":
    srcs = sys.argv[1:] or B.SOURCES
    with ThreadPoolExecutor(max_workers=8) as ex:
        for rows in ex.map(listing, srcs):
            print("\n".join(rows))
