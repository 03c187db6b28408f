"""The IA_* environment switches the package and its kernels read == the first column of the table in INTEGRATION.md section 5.
Regular expressions over source text only: nothing of the package is imported."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "intrinsicavatar_amd")

# os.environ.get("IA_X" / os.environ["IA_X"] / os.environ.setdefault("IA_X" / "IA_X" in os.environ / getenv("IA_X")
READS = [re.compile(r'environ\s*(?:\.\s*\w+\s*\(|\[)\s*["\'](IA_[A-Z0-9_]+)["\']'),
         re.compile(r'["\'](IA_[A-Z0-9_]+)["\']\s+(?:not\s+)?in\s+(?:\w+\.)?environ'),
         re.compile(r'getenv\s*\(\s*["\'](IA_[A-Z0-9_]+)["\']')]


def names_read():
    found = {}
    for d, _, files in os.walk(PKG):
        for f in files:
            if not f.endswith((".py", ".hip", ".h")):
                continue
            with open(os.path.join(d, f), encoding="utf-8") as fh:
                text = fh.read()
            for rx in READS:
                for name in rx.findall(text):
                    found.setdefault(name, set()).add(f)
    return found


def integration_sections():
    """(names of the table's first column, text of the retired list) of INTEGRATION.md's section on the run-time switches."""
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as fh:
        text = fh.read()
    sec = re.search(r"^## 5\. Run-time switches.*?(?=^## |\Z)", text, re.S | re.M)
    assert sec, "INTEGRATION.md has no section '5. Run-time switches'"
    table, _, retired = sec.group(0).partition("\nRetired")
    rows = re.findall(r"^\|\s*`(IA_[A-Z0-9_]+)`\s*\|", table, re.M)
    return rows, retired


def test_the_table_lists_exactly_the_switches_the_source_reads():
    read = names_read()
    rows, _ = integration_sections()
    assert len(rows) == len(set(rows)), sorted(n for n in rows if rows.count(n) > 1)
    undocumented = {n: sorted(read[n]) for n in set(read) - set(rows)}
    stale = sorted(set(rows) - set(read))
    assert not undocumented and not stale, f"read but not in the table: {undocumented}; in the table but read nowhere: {stale}"
    assert len(rows) >= 20                  # the patterns above found the reads at all


def test_no_retired_name_is_still_read():
    read = names_read()
    _, retired = integration_sections()
    names = set(re.findall(r"`(IA_[A-Z0-9_]+)`", retired))
    assert names, "the retired list is empty"
    assert not names & set(read), sorted(names & set(read))
