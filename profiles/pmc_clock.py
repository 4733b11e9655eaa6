"""pmc_clock.py DIR [kernel-name-substring ...]: the clock the chip held under each kernel, from the csv output of a counter pass
`rocprofv3 --pmc GRBM_GUI_ACTIVE --output-format csv -d DIR -- <program>`: GRBM_GUI_ACTIVE / 8 (the counter is summed over the 8 XCDs) / wall time of
the dispatch, over the dispatches of 0.3 ms and more (the quotient reads high on shorter ones)."""
import collections
import csv
import glob
import sys


def main():
    d, subs = sys.argv[1], sys.argv[2:]
    rows = collections.defaultdict(list)
    for f in glob.glob(d + "/**/*counter_collection*.csv", recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                name = r.get("Kernel_Name", "?")
                if r.get("Counter_Name") != "GRBM_GUI_ACTIVE" or (subs and not any(s in name for s in subs)):
                    continue
                rows[name].append((float(r["Counter_Value"]), float(r["End_Timestamp"]) - float(r["Start_Timestamp"])))
    for name, v in rows.items():
        v = [x for x in v if x[1] > 3e5] or v
        ghz = sorted(c / 8 / w for c, w in v)
        print("%-90s n=%3d wall %8.1f us  clock GHz min %.3f med %.3f max %.3f"
              % (name[:90], len(v), sum(w for _, w in v) / len(v) / 1e3, ghz[0], ghz[len(ghz) // 2], ghz[-1]))


if __name__ == "__main__":
    main()
