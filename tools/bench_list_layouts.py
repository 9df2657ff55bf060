"""Host time of the five list passes' layouts (the `imgxf_*_layout_host` calls; no device) on the corpus of
tests/golden/make_list_layout_golden.py: the median of `--calls` timed calls (size call + fill call) per pass and
parameter set, one JSON line.  IMGXF_LIBRARY selects the library, so the same script times a parent build: run the two
alternately, three processes each, and hold the candidate's median of medians against the parent's own spread
(profiles/list_layout.txt).

    IMGXF_LIBRARY=/path/to/libimgxf.so python tools/bench_list_layouts.py --label parent"""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="candidate")
    ap.add_argument("--calls", type=int, default=21)
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("golden", os.path.join(ROOT, "tests", "golden", "make_list_layout_golden.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    corpus = G.corpus()
    out = {"label": args.label, "calls": args.calls, "median_ms": {}}
    for key, make in G.layouts(corpus):
        if key.endswith("/n0"):
            continue
        make()                                               # first touch of the pages and of the code
        times = []
        for _ in range(args.calls):
            t = time.perf_counter()
            make()
            times.append(time.perf_counter() - t)
        out["median_ms"][key] = round(sorted(times)[len(times) // 2] * 1e3, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
