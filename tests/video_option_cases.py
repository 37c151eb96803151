"""The option combinations of the streamed-video path, for both front ends: one representative valid value per option of
VideoInterpolator and of scripts/interpolate_video.py, every single, pair and triple of them, and what running one gives - accepted, or
the refusal with its full text.  tests/golden/make_video_refusals.py records the outcomes of a commit, tests/test_video_option_table_cpu.py
compares the working tree's with them.  Nothing here needs a GPU: the constructor and getargs() only look at their arguments.

A plain helper module (no fixtures, no collection hooks), imported as tests/video_clips.py is."""
import argparse
import configparser
import itertools

# option -> the constructor's keyword value; "recurrent" is no keyword: the model says it
API_VALUES = {
    "upsample_rate": 3,
    "target_rate": (60, 1),
    "speed": "1/2",
    "shutter": "1/2",
    "scene_cut": "1/10",
    "shutter_light": "bt709",
    "shutter_window": "hann",
    "deinterlace": "tff",
    "dedup": True,
    "active": "auto",
    "field_probe": True,
    "static": 0,
    "flow_check": True,
    "flow_alpha": 0.02,
    "flow_scale": 2,
    "tile": (64, 64),
    "recurrent": True,
}

# option -> the command line's words; flow_alpha and a recurrent model have no flag, --slowmo and --detelecine no constructor argument
FLAG_VALUES = {
    "upsample_rate": ["--upsample_rate", "3"],
    "target_rate": ["--fps", "60"],
    "speed": ["--speed", "1/2"],
    "shutter": ["--shutter", "180"],
    "scene_cut": ["--scene_cut", "1/10"],
    "shutter_light": ["--shutter_light", "bt709"],
    "shutter_window": ["--shutter_window", "hann"],
    "deinterlace": ["--deinterlace", "tff"],
    "dedup": ["--dedup"],
    "active": ["--active", "auto"],
    "field_probe": ["--field_probe"],
    "static": ["--static", "0"],
    "flow_check": ["--flow_check"],
    "flow_scale": ["--flow_scale", "2"],
    "tile": ["--tile", "64x64"],
    "slowmo": ["--slowmo"],
    "detelecine": ["--detelecine"],
}

BASE = ["-c", "x.ini", "--expt", "e", "--log", "l", "--input", "-", "--output", "-"]


def cases(values):
    """Every single, pair and triple of the options of `values`, as tuples of names in the order of `values`."""
    return [c for n in (1, 2, 3) for c in itertools.combinations(values, n)]


def case_id(names):
    return "+".join(names)


class _Model:
    recurrent = False
    precision = None


class _Recurrent(_Model):
    recurrent = True


def _cfg():
    cfg = configparser.RawConfigParser()
    cfg.read_dict({"TRAIN": {"N_FRAMES": "2"}})
    return cfg


def api_outcome(V, names):
    """None where VideoInterpolator takes the options `names`, else [exception type's name, full message]."""
    kw = {k: API_VALUES[k] for k in names if k != "recurrent"}
    try:
        V.VideoInterpolator((_Recurrent if "recurrent" in names else _Model)(), _cfg(), **kw)
    except Exception as e:
        return [type(e).__name__, str(e)]
    return None


class _Refused(Exception):
    pass


def flag_outcome(tool, names):
    """None where getargs() takes the flags of `names`, else the text it handed to parser.error (the usage line and the program's name
    that argparse puts around it are the caller's, not the tool's)."""
    def error(self, message):
        raise _Refused(message)
    kept, argparse.ArgumentParser.error = argparse.ArgumentParser.error, error
    try:
        tool.getargs(BASE + [word for k in names for word in FLAG_VALUES[k]])
    except _Refused as e:
        return str(e)
    finally:
        argparse.ArgumentParser.error = kept
    return None


def outcomes(V, tool):
    """({case id: outcome} of the constructor, the same of the tool), every case of both front ends."""
    return ({case_id(c): api_outcome(V, c) for c in cases(API_VALUES)}, {case_id(c): flag_outcome(tool, c) for c in cases(FLAG_VALUES)})
