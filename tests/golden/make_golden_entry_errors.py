"""Records tests/golden/g23_entry_errors.json: what every case of tests/entry_error_cases.py answers (status and message
of the C entry point, exception type and text of the Plan method), and, with no device needed, the signature and
docstring of the 16 sampler methods of Plan and every _lib.SYMBOLS entry by the names of its types.

    python tests/golden/make_golden_entry_errors.py [output.json]      (on the GPU)

The record is the surface a change of the host code must keep: it is made ONCE, at the commit whose behaviour is to be
kept, and not regenerated with the code under test."""
import inspect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import entry_error_cases as E  # noqa: E402


def host_surface():
    from eeyore_amd import _lib as L
    from eeyore_amd.plan import Plan
    return dict(signatures={m: str(inspect.signature(getattr(Plan, m))) for m in E.PLAN_METHODS},
                docs={m: getattr(Plan, m).__doc__ for m in E.PLAN_METHODS},
                symbols={k: E.symbol_text(v) for k, v in L.SYMBOLS.items()})


def device_records(device="cuda:0"):
    out = {}
    for name in E.WORLDS:
        w = E.World(name, device)
        for entry in E.ENTRIES:
            for case in E.c_cases(entry):
                if name in case.worlds:
                    rc, msg = E.run_c(w, entry, case)
                    assert (rc == 0) <= (case.mut.get("C") == 0), (entry, case.name, "was served")
                    assert rc != 0 or msg == "", (entry, case.name)
                    out[E.record_key("c", entry, name, case.name)] = dict(status=rc, message=msg)
        for entry, method, base in E.plan_entries():
            for case in E.plan_cases(entry):
                if name in case.worlds:
                    exc, text = E.run_plan(w, method, base, case)
                    assert exc, (entry, case.name, "was served")
                    out[E.record_key("plan", entry, name, case.name)] = dict(exception=exc, text=text)
        assert w.changed() == [], w.changed()
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else E.GOLDEN
    rec = dict(host_surface(), cases=device_records())
    E.dump_record(rec, path)
    print(f"{len(rec['cases'])} cases -> {path}")
