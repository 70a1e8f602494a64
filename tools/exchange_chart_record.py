"""Rewrites tests/golden/exchange_chart.json, the record of the exchange chart (tests/exchange_chart.py): seeds, per case
the shard rows and padding rows, a sha256 of all ranks' shards, of the model's blocks in each wire form and of the hazard
binary16 gather buffer, and the census counts (CPU only).

  python tools/exchange_chart_record.py

tests/test_exchange_chart.py compares the chart with this record, so that the population cannot drift unnoticed."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PATH = os.path.join(ROOT, "tests", "golden", "exchange_chart.json")

if __name__ == "__main__":
    import exchange_chart as X
    with open(PATH, "w") as f:
        json.dump(X.record(), f, indent=1)
        f.write("\n")
    print("wrote", PATH)
