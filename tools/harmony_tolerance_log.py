"""Writes profiles/harmony_tolerances.log from the figures that the Harmony tests record (tests/harmony_cases.py:record):
    SCAMD_HARMONY_RECORDS=emu.tsv python -m pytest tests/test_emu_harmony_cpu.py                                   (any host)
    SCAMD_HARMONY_RECORDS=gpu.tsv python -m pytest -m gpu tests/test_gpu_harmony.py tests/test_gpu_harmony_pipeline.py   (MI355X)
    python tools/harmony_tolerance_log.py emu.tsv gpu.tsv > profiles/harmony_tolerances.log"""
import sys


def read(path):
    rows = {}
    for line in open(path):
        label, case, quantity, sens, bnd, dev = line.rstrip("\n").split("\t")
        key = (case, quantity)
        # (a comparison made twice, as by a rerun, keeps its larger deviation)
        if key not in rows or float(dev) > float(rows[key][2]):
            rows[key] = (sens, bnd, dev)
    return rows


emu, gpu = read(sys.argv[1]), read(sys.argv[2])
keys = list(emu) + [k for k in gpu if k not in emu]
print("# Tolerances of the Harmony tests (tests/harmony_cases.py; written by tools/harmony_tolerance_log.py).  Per case and quantity: the")
print("# round-off sensitivity of the CPU truth (largest |float64 run - longdouble run|), the bound (16 x that, at least 1e-12 of the largest")
print("# entry; 'z_hat vs lstsq' is held to the bound of z_hat; the two invariants after init and after every round, 'sum O - sum R' and")
print("# 'E - pr_b sum R', to 1e-12 of the largest column sum / entry, at least of 1: they have no sensitivity), and the largest")
print("# deviation of the kernels on the host emulator and on the MI355X.")
print(f"{'case':<44}{'quantity':<26}{'sensitivity':>12}{'bound':>12}{'emulator':>12}{'MI355X':>12}")
worst = 0.0
for k in keys:
    sens, bnd, _ = emu.get(k) or gpu[k]
    devs = [rows[k][2] if k in rows else "-" for rows in (emu, gpu)]
    for rows in (emu, gpu):
        if k in rows and float(rows[k][1]) > 0:
            worst = max(worst, float(rows[k][2]) / float(rows[k][1]))
    print(f"{k[0]:<44}{k[1]:<26}{('-' if sens == 'nan' else sens):>12}{bnd:>12}{devs[0]:>12}{devs[1]:>12}")
print(f"# largest deviation / bound over all rows: {worst:.3f}")
