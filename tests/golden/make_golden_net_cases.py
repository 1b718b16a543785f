"""Records tests/golden/net_cases_parent.json: per net (blocked, step, impute, gram, ssm_net, pmf_net, bpmf_net) and per case index, the SHA-256 of
the case dict and of the arrays of problem(device_case(i)) (tests/test_net_cases_unchanged_cpu.py, which holds the digests' definition).
Run once, without a GPU, at the commit whose cases are to be kept:

    python tests/golden/make_golden_net_cases.py tests/golden/net_cases_parent.json"""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_net_cases_unchanged_cpu as TN       # noqa: E402


def main():
    rec = {}
    for net in sorted(TN.NETS):
        rec[net] = TN.record(net)
        print(f"{net}: {len(rec[net])} cases", flush=True)
    with open(sys.argv[1], "w") as f:          # one net per line
        f.write("{\n" + ",\n".join(f"{json.dumps(net)}: {json.dumps(rec[net])}" for net in sorted(rec)) + "\n}\n")


if __name__ == "__main__":
    main()
