"""CPU: the reference's printed event table of its single test read (test/ecoli_2kb_region/single_read/read1.events.exp, minted into
tests/golden/read1_events.npz by make_read1_events.py) is reproduced by the oracle's getevents from the read's raw signal: start and
length exactly, mean and stdv in every printed decimal.  The GPU side of the same pin is tests/test_event_fields.py.  Also pins the
values of the ABEA_EV_FIELDS_* constants of include/abea.h in C and C++, and their Python mirrors."""
import os
import subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_oracle_getevents_reproduces_the_printed_read1_table(orc):
    g = np.load(os.path.join(GOLD, "read1_events.npz"))
    assert len(g["signal"]) == 36121 and len(g["start"]) == 7165
    ev, _ = orc.getevents(g["signal"], *[float(x) for x in g["scaling"]])
    assert len(ev) == 7165
    assert (ev["start"] == g["start"]).all() and (ev["length"] == g["length"]).all()
    assert [b"%.6f" % x for x in ev["mean"]] == list(g["mean_txt"])
    assert [b"%.6f" % x for x in ev["stdv"]] == list(g["stdv_txt"])
    # the events tile the signal (events.c:466-513), which is what lets the narrow table records drop `length`
    assert g["start"][0] == 0 and int(g["start"][-1]) + int(g["length"][-1]) == len(g["signal"])
    assert (g["start"][1:] == g["start"][:-1] + g["length"][:-1].astype(np.uint64)).all()


PIN = r"""
#include "abea.h"
#include "abea_f5c_shim.h"
#if ABEA_EV_FIELDS_ALL != 0u || ABEA_EV_FIELDS_NO_STDV != 1u || ABEA_EV_FIELDS_LAYOUT != 2u
#error "ABEA_EV_FIELDS_* changed"
#endif
typedef int (*ev_fn)(abea_ctx*, const abea_events_host_batch*, uint32_t);
typedef int (*pr_fn)(abea_ctx*, const abea_process_batch*, uint32_t);
typedef void (*shim_fn)(abea_f5c_core*, abea_f5c_db*, uint32_t);
int main(void) {
    ev_fn a = abea_events_batch_host_fields; pr_fn b = abea_process_batch_host_fields;
    shim_fn c = abea_f5c_event_db_fields, d = abea_f5c_process_fields;
    return !(a && b && c && d);
}
"""


def test_ev_fields_constants_are_pinned(tmp_path):
    from f5c_amd import abea
    assert (abea.EV_FIELDS_ALL, abea.EV_FIELDS_NO_STDV, abea.EV_FIELDS_LAYOUT) == (0, 1, 2)
    src = tmp_path / "pin.c"
    src.write_text(PIN)
    for cmd in (["gcc", "-std=c11"], ["g++", "-x", "c++", "-std=c++11"]):
        r = subprocess.run(cmd + ["-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, f"{cmd[0]}:\n{r.stderr[-3000:]}"
