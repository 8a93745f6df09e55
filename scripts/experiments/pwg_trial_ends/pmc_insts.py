"""Instructions per env step of the headline's timed launches, from one rocprofv3 counter pass of
`bench.py --gpus 1 --steps 4 --warmup 1` (C3: 65 536 instances x 512 steps per launch):

    rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_LDS \
        SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAVES -d DIR -o p --output-format csv -- python bench.py ...
    python scripts/experiments/pwg_trial_ends/pmc_insts.py DIR/.../p_counter_collection.csv

The last four dispatches of k_tab_pwg are the timed ones (everything before is pre-training)."""
import csv
import sys


def main():
    rows = {}
    with open(sys.argv[1], newline='') as fh:
        for r in csv.DictReader(fh):
            if 'k_tab_pwg' not in r['Kernel_Name']:
                continue
            d = rows.setdefault(int(r['Dispatch_Id']), {})
            d[r['Counter_Name']] = d.get(r['Counter_Name'], 0.0) + float(r['Counter_Value'])
    timed = [rows[k] for k in sorted(rows)[-4:]]
    steps = 65536 * 512 * len(timed)
    print('dispatches of k_tab_pwg: %d, timed: %d' % (len(rows), len(timed)))
    for name in sorted(timed[0]):
        print('%-18s %10.3f per env step' % (name, sum(t[name] for t in timed) / steps))


if __name__ == '__main__':
    main()
