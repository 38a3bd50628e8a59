"""The recorder the parent-bits tests share: a golden JSON file {"commit", "what", "digests": case id -> digest(s)} under
tests/golden/.  What a case is and how its output is digested is each test file's own."""
import json
import os
import subprocess
import sys


def load(golden):
    with open(golden) as f:
        return json.load(f)["digests"]


def save(golden, commit, what, digests):
    doc = {"commit": commit, "what": what, "digests": digests}
    with open(golden, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return doc


def names_match(golden, case_ids):
    """The record names every case and nothing else"""
    return sorted(load(golden)) == sorted(case_ids)


def main(record, source=""):
    """A test file run as a program: record(commit) at the commit given as the first argument, else at HEAD"""
    head = sys.argv[1] if len(sys.argv) > 1 else subprocess.run(["git", "rev-parse", "HEAD"], cwd=os.path.dirname(os.path.abspath(__file__)), check=True,
                                                                stdout=subprocess.PIPE, text=True).stdout.strip()
    print(f"{len(record(head)['digests'])} cases recorded at {head}{source}")
