"""The "[acc]" lines of `pytest -m gpu tests/test_gpu_accuracy.py -s` -> profiles/accuracy/accuracy_budget.json
and the per-stage table of that test's docstring.

  python tools/acc_lines.py pytest.log [out.json]

Each line reads "[acc] stage shape arithmetic what max_ratio=.. rms_ratio=.. e_ref_max=.. e_max=..": the
ratio of the device's error to the float32 reference's, both against float64 (tests/f64_ref.py).
The log-mel front end has two lines per case, "log" and "lin" (the log output, and exp(out) over the
frame's largest float64 mel power); its shape is case-form (form q16 or wave), and the arithmetic
column only names the engine that ran it.  The beam lines are one per case (B, k, weights).

A log of tests/test_gpu_configs.py has the same lines, the shape column naming the configuration and the
case (V4-fold, l8r1-per-step, L1-B3k8, ...), and goes to profiles/accuracy/accuracy_budget_configs.json:

  python tools/acc_lines.py pytest_configs.log profiles/accuracy/accuracy_budget_configs.json

A log of tests/test_gpu_accuracy_s16x1.py (arithmetic s16x1) has a second line per quantity,
"[acc] stage shape s16x1 what cost e_dev_max=.. e_dev_rms=.. e_model_max=.. e_model_rms=..": the
device's and the float64 s16x1 model's distance from the unrounded float64 stage.  Its ratios are to the
float32 evaluation of that model, its table has one column pair and the cost, and it goes to
profiles/accuracy/accuracy_budget_s16x1.json:

  python tools/acc_lines.py pytest_s16x1.log profiles/accuracy/accuracy_budget_s16x1.json

A log of tests/test_gpu_convert.py has one line per (rate x channels) case of casr_convert_audio, stage
"convert" (the arithmetic column reads f32: no MFMA is involved); its ratios are to the float32
restatement of tests/resample_ref.py, and it goes to profiles/convert/accuracy.json:

  python tools/acc_lines.py pytest_convert.log profiles/convert/accuracy.json"""
import json
import re
import sys

LINE = re.compile(r"\[acc\] (\S+) (\S+) (s16x3|f32|s16x1) (\S+) max_ratio=(\S+) rms_ratio=(\S+) e_ref_max=(\S+) e_max=(\S+)")
COST = re.compile(r"\[acc\] (\S+) (\S+) (s16x1) (\S+) cost e_dev_max=(\S+) e_dev_rms=(\S+) e_model_max=(\S+) "
                  r"e_model_rms=(\S+)")


def parse(text):
    cost = {m.group(1, 2, 3, 4): [float(x) for x in m.group(5, 6, 7, 8)] for m in COST.finditer(text)}
    rows = []
    for m in LINE.finditer(text):
        stage, shape, arith, what = m.group(1, 2, 3, 4)
        mx, rms, eref, emax = (float(x) for x in m.group(5, 6, 7, 8))
        rows.append(dict(stage=stage, shape=shape, arithmetic=arith, what=what, max_ratio=mx, rms_ratio=rms,
                         e_ref_max=eref, e_max=emax))
        if (stage, shape, arith, what) in cost:
            rows[-1].update(zip(("cost_dev_max", "cost_dev_rms", "cost_model_max", "cost_model_rms"),
                                cost[(stage, shape, arith, what)]))
    return rows


def table_s16x1(rows):
    """Per stage and quantity: the largest ratios to the float32 model's error over the cases, the worst
    shape, and the largest distance of the device (and of the float64 model) from the unrounded stage."""
    keys, best = [], {}
    for r in rows:
        k = (r["stage"], r["what"])
        if k not in keys:
            keys.append(k)
        b = best.setdefault(k, dict(max_ratio=0.0, rms_ratio=0.0, shape=None, n=0, dev=0.0, model=0.0))
        b["n"] += 1
        b["rms_ratio"] = max(b["rms_ratio"], r["rms_ratio"])
        b["dev"], b["model"] = max(b["dev"], r.get("cost_dev_max", 0.0)), max(b["model"], r.get("cost_model_max", 0.0))
        if r["max_ratio"] >= b["max_ratio"]:
            b["max_ratio"], b["shape"] = r["max_ratio"], r["shape"]
    out = [f"  {'stage':9s}{'quantity':12s}{'cases':>6s}  {'max':>6s} {'rms':>6s}  {'worst shape':24s} {'cost: device':>13s} {'model':>9s}"]
    for k in keys:
        b = best[k]
        out.append(f"  {k[0]:9s}{k[1]:12s}{b['n']:6d}  {b['max_ratio']:6.2f} {b['rms_ratio']:6.2f}  {b['shape']:24s} "
                   f"{b['dev']:13.1e} {b['model']:9.1e}")
    return "\n".join(out)


def table(rows):
    """Per stage and quantity, the largest ratios over the shapes, one column pair per arithmetic."""
    keys = []
    best = {}
    for r in rows:
        k = (r["stage"], r["what"])
        if k not in keys:
            keys.append(k)
        b = best.setdefault(k + (r["arithmetic"],), dict(max_ratio=0.0, rms_ratio=0.0, shape=None, n=0))
        b["n"] += 1
        b["rms_ratio"] = max(b["rms_ratio"], r["rms_ratio"])
        if r["max_ratio"] >= b["max_ratio"]:
            b["max_ratio"], b["shape"] = r["max_ratio"], r["shape"]
    out = [f"  {'stage':9s}{'quantity':12s}{'cases':>6s}  {'s16x3 max':>9s} {'rms':>6s}  {'f32 max':>9s} {'rms':>6s}  worst shape (s16x3 / f32)"]
    for k in keys:
        a, b = best.get(k + ("s16x3",)), best.get(k + ("f32",))
        out.append(f"  {k[0]:9s}{k[1]:12s}{a['n']:6d}  {a['max_ratio']:9.2f} {a['rms_ratio']:6.2f}  "
                   f"{b['max_ratio']:9.2f} {b['rms_ratio']:6.2f}  {a['shape']} / {b['shape']}")
    return "\n".join(out)


if __name__ == "__main__":
    rows = parse(open(sys.argv[1], encoding="utf-8").read())
    x1 = bool(rows) and all(r["arithmetic"] == "s16x1" for r in rows)
    if rows and all(r["stage"] == "convert" for r in rows):
        if len(sys.argv) > 2:
            with open(sys.argv[2], "w", encoding="utf-8") as f:
                json.dump(dict(margin=8, reference="float64 (tests/resample_ref.py); ratios are to the float32 "
                               "restatement's error on the same inputs (quantize = 0, normalisation off)",
                               device="MI355X (gfx950)", cases=rows), f, indent=1)
                f.write("\n")
        for r in rows:
            print(f"  {r['shape']:10s} max {r['max_ratio']:6.3f} rms {r['rms_ratio']:6.3f}  e_ref_max {r['e_ref_max']:.3e}")
        sys.exit(0)
    if x1:
        if len(sys.argv) > 2:
            with open(sys.argv[2], "w", encoding="utf-8") as f:
                json.dump(dict(margin=8, reference="the float64 s16x1 model (tests/f64_ref.py, sites); ratios are to the "
                               "float32 evaluation of the same model on the same stage inputs; cost_*: distance from "
                               "the unrounded float64 stage, of the device and of the float64 model",
                               device="MI355X (gfx950)", cases=rows), f, indent=1)
                f.write("\n")
        print(table_s16x1(rows))
        sys.exit(0)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w", encoding="utf-8") as f:
            json.dump(dict(margin=8, reference="float64 (tests/f64_ref.py); ratios are to the float32 oracle's error "
                           "on the same stage inputs", device="MI355X (gfx950)", cases=rows), f, indent=1)
            f.write("\n")
    print(table(rows))
