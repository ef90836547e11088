"""What tests/test_stats_cases.py, tests/test_gpu_color_stats.py and tests/golden/make_stats_cases.py share: the option sets a catalogue
file is decoded under, and one walk over a case's passes on any backend of oracle/harness.py."""
import numpy as np

import stats_model as SM

# name -> (options of the decode, histo_en as the model sees it)
OPTION_SETS = {"histo": (dict(decode_ac=1, histo_en=1), 1), "clip": (dict(decode_ac=1, stat_clip_en=1), 0),
               "histo_dc": (dict(decode_ac=0, histo_en=1), 1), "clip_dc": (dict(decode_ac=0, stat_clip_en=1), 0)}


def words(b):
    st = b.color_stats()
    return np.concatenate([st["histo"].view(np.uint32), np.array([st["count"]], np.uint32), st["clip"], st["rgb"].ravel(), st["yfull"]])


def recorded_log(rec, key):
    """The clip warnings tests/golden/stats_cases.json keeps for option set `key`, per pass."""
    log = rec["log"]
    return log["all"] if "all" in log else log["full" if OPTION_SETS[key][0]["decode_ac"] else "dc"]


def clip_lines(lines):
    return [l for l in lines if "YCC Clipped" in l or "Only reported first" in l]


def run_passes(H, b, case, key, keep=False, probe=None):
    """Decodes case.file on backend b under option set `key`, then makes the case's re-renders.  Per pass: the record (`words`), its digest, the
    clip warnings the pass logged (the oracle keeps no log) and the digest of the DIB; with keep, the DIBs and the planes themselves; with probe,
    what probe(b) answers right behind the decode."""
    opt, _ = OPTION_SETS[key]
    out = {"words": [], "digest": [], "log": [], "dib": [], "dibs": [], "planes": None}
    b.set_options(**opt)
    try:
        H.drive(b, case.file)
        out["probe"] = probe(b) if probe else None
        seen = 0
        for p in range(1 + len(case.rerenders)):
            if p:
                b.set_preview_ycc_offset(*case.rerenders[p - 1])
            dib = b.dib()
            assert dib is not None, "%s [%s]: no DIB on %s" % (case.name, key, b.name)
            w = words(b); lines = b.log_lines()
            out["words"].append(w); out["digest"].append(H.hash_bytes(w)[:16]); out["dib"].append(H.hash_bytes(dib)[:16])
            out["log"].append(clip_lines(lines[seen:])); seen = len(lines)
            if keep:
                out["dibs"].append(dib)
                if p == 0:
                    out["planes"] = b.planes()
        if case.rerenders:
            b.set_preview_ycc_offset(0, 0, 0, 0, 0)
    finally:
        b.set_options()
    return out


def explain(case, key, p, got, res):
    """The failure message for a record that differs from the model's (res = case.model(...)) after pass p: the first differing word by meaning and,
    for a YCC clip counter, the model's first event of the pass that the counters leave out or the kind they have too many of."""
    from stats_cases import CLIP_STEP, SWEEP
    d = SM.first_difference(got, res.records[p])
    if d is None:
        return None
    k, name, g, e = d
    msg = "%s [%s] pass %d: %s is %d, expected %d (word %d)" % (case.name, key, p, name, g, e, k)
    if 37 <= k < 43:
        before = res.records[p - 1][37:43].astype(np.int64) if p else np.zeros(6, np.int64)
        have = np.asarray(got[37:43], np.int64) - before                   # what the library counted in this pass, by kind
        for (pix, mcu, kind, vals) in res.events[p]:
            w = SM.KIND_CLIP_WORD[SM.KINDS.index(kind)]
            if have[w] <= 0:
                msg += "; the model's first event the counters miss: pixel %d (pixel %% %d = %d, pixel // SWEEP = %d) MCU %s %s %s" % (
                    pix, CLIP_STEP, pix % CLIP_STEP, pix // SWEEP, mcu, kind, vals)
                break
            have[w] -= 1
        else:
            extra = [SM.CLIP_NAMES[i] for i in range(6) if have[i] > 0]
            msg += "; counted besides the model's %d events of the pass: %s" % (len(res.events[p]), extra)
    return msg
