"""Registers, scratch and audit counts of the GP4 kernels in a directory of listings
(tools/compare_device_code.py --listings <tree> <dir>), one line per kernel:

    python tools/gp4_listing_stats.py <dir>

vgpr / agpr / sgpr / scratch bytes / LDS bytes come from the kernel's metadata, the rest is the
report line of tools/audit_gp4.py::audit (k_gp_sweep4) or plain counts (k_gp_mean_blocks).
"""
import glob
import os
import re
import sys

import audit_gp4

FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def metadata(text):
    """{kernel: {field: value}} from the amdhsa.kernels metadata of a listing."""
    out = {}
    for entry in re.split(r"\n  - ", text.split("amdhsa.kernels:")[1]):
        name = re.search(r"\.name:\s+(\S+)", entry)
        if name:
            out[name.group(1)] = {f: int(re.search(re.escape(f) + r":\s+(\d+)", entry).group(1)) for f in FIELDS}
    return out


def main(directory):
    for dim in (1, 2, 3, 4):
        for stem, prefix in (("sl_gp4_d%d" % dim, "_Z11k_gp_sweep4"), ("sl_gp4_mean_d%d" % dim, "_Z16k_gp_mean_blocks")):
            path = glob.glob(os.path.join(directory, stem, "*.s"))[0]
            text = open(path).read()
            # (the build's audit arguments for k_gp_sweep4; k_gp_mean_blocks owns no accumulator register)
            sweep = "sweep4" in prefix
            lines = dict(l.split(": ", 1) for l in audit_gp4.audit(path, prefix, 4 if sweep else 0, 128 if sweep else 0)[0])
            for name, m in sorted(metadata(text).items()):
                if name.startswith(prefix):
                    print("%s %s: vgpr %d agpr %d sgpr %d scratch %d B lds %d B; %s"
                          % (stem, name, *[m[f] for f in FIELDS], lines[name]))


if __name__ == "__main__":
    main(sys.argv[1])
