"""Median dispatch time of the three beam kernels (and the greedy pick) from a `rocprofv3 --kernel-trace` CSV of `scripts/beam_step.py --short`:
`python scripts/beam_trace_medians.py <dir with *_kernel_trace.csv> OUT.json`."""
import csv
import glob
import json
import os
import sys

NAMES = ('beam_cand_kernel', 'beam_select_kernel', 'beam_reorder_kernel', 'pick_kernel')


def main(d, out):
    t = {n: [] for n in NAMES}
    for f in glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True):
        for r in csv.DictReader(open(f)):
            for n in NAMES:
                if n in r['Kernel_Name']:
                    t[n].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    res = {n: {'dispatches': len(v), 'median_us': round(sorted(v)[len(v) // 2], 1), 'max_us': round(max(v), 1)} for n, v in t.items() if v}
    with open(out, 'w') as fh:
        fh.write(json.dumps(res, indent=1) + '\n')
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
