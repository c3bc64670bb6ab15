#!/usr/bin/env python3
"""The commands of a rocprofv3 --kernel-trace --memory-copy-trace run (csv), stream by stream in the order they were issued:
what two builds must agree on when a change may not move a command.

  python tools/trace_commands.py DIR/t_kernel_trace.csv DIR/t_memory_copy_trace.csv > listing.txt
  python tools/trace_commands.py --compare a.txt b.txt          exit status 0: the same counts and the same order per stream

The listing: a legend (index, count, name -- a kernel's name without its arguments, a copy's direction), then one line per
stream: its commands as legend indices in issue order (the API call's correlation id), `k*i` for k in a row."""
import collections
import csv
import sys


def commands(kernels, copies):
    rows = []
    with open(kernels, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"].replace("void ", "").replace("(anonymous namespace)::", "")
            rows.append((int(r["Correlation_Id"]), int(r["Stream_Id"]), name.split("(")[0]))
    with open(copies, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Correlation_Id"]), int(r["Stream_Id"]), r["Direction"]))
    return sorted(rows)


def listing(rows):
    count = collections.Counter(name for _, _, name in rows)
    index = {name: i for i, name in enumerate(sorted(count))}
    out = ["# commands by name: index count name"] + ["%d %d %s" % (index[n], count[n], n) for n in sorted(count)]
    streams = collections.defaultdict(list)
    for _, s, name in rows:
        streams[s].append(index[name])
    out.append("# streams in order of creation: stream commands | sequence")
    for s in sorted(streams):
        seq, runs = streams[s], []
        for i in seq:
            if runs and runs[-1][0] == i:
                runs[-1][1] += 1
            else:
                runs.append([i, 1])
        out.append("%d %d | %s" % (s, len(seq), " ".join("%d*%d" % (k, i) if k > 1 else str(i) for i, k in runs)))
    return "\n".join(out) + "\n"


def main():
    if sys.argv[1] == "--compare":
        a, b = (open(p).read() for p in sys.argv[2:4])
        if a == b:
            print("equal: counts by name and order on every stream")
            return 0
        for k, (x, y) in enumerate(zip(a.splitlines(), b.splitlines())):
            if x != y:
                print("first difference, line %d:\n  %s\n  %s" % (k + 1, x[:300], y[:300]))
                break
        return 1
    sys.stdout.write(listing(commands(sys.argv[1], sys.argv[2])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
