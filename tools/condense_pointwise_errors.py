"""The rows tests/test_train_pointwise_gpu.py appends to the file ISR_TRAIN_POINTWISE_REPORT names -> the table of
profiles/train_pointwise_errors.md on stdout: per (case without its AO / previous-frame variant, pixel set) the row closest to its bar, the
number of rows it stands for and the largest error among them.  The loss's sixteen scalar values are one set, Adam's five updates one.

    ISR_TRAIN_POINTWISE_REPORT=rows.md python -m pytest tests/test_train_pointwise_gpu.py && python tools/condense_pointwise_errors.py rows.md"""
import re
import sys
from collections import OrderedDict

rows = OrderedDict()
for line in open(sys.argv[1]):
    parts = [p.strip() for p in line.strip().strip("|").split("|")]
    if len(parts) != 5:
        continue
    case, kind, err, own, bar = parts
    err, own, bar = float(err), float(own), float(bar)
    key_case = re.sub(r" ao \d\.\d\d inv \d prev (gradient|no gradient|absent)", "", case)
    if re.match(r"^(mse|l1|temp-l2):|^total$", kind):
        kind = "term values and total"
    if kind.startswith("update / lr"):
        kind = "update / lr (five steps)"
    key = (key_case, kind)
    ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
    cur = rows.get(key)
    if cur is None:
        rows[key] = [err, own, bar, ratio, 1, err]
    else:
        cur[4] += 1
        cur[5] = max(cur[5], err)
        if ratio > cur[3]:
            cur[0:4] = [err, own, bar, ratio]
for (case, kind), (err, own, bar, ratio, count, worst) in rows.items():
    print("| %s | %s | %d | %.2e | %.2e | %.2e | %.2e |" % (case, kind, count, worst, err, own, bar))
