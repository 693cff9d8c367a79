"""Which environment switches a source file of the library reads.  A diagnostic or a test hook is read where it is used (isle_ctx::knob,
knob_on); a switch that selects or tunes a form is read through its typed value: a field of RouteEnv (isle_amd/csrc/route_host.h), named
after the switch, either directly (c->route.<field>) or inside a rule of route_host.h that the file calls.  The coverage guards of the
certificates (gram_certificate.py, infer_certificate.py) ask this module, so that a switch a kernel's route depends on cannot go unswept."""
import os
import re

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(_ROOT, "isle_amd", "csrc")


def knob_ids():
    """[KN_...] in the order of the switch table (knobs.h IsleKnob)."""
    text = open(os.path.join(_SRC, "knobs.h")).read()
    body = re.search(r"enum IsleKnob \{(.*?)\};", text, flags=re.S).group(1)
    ids = [t.strip() for t in body.replace("\n", " ").split(",") if t.strip()]
    assert ids[-1] == "KN_COUNT"
    return ids[:-1]


def _field_to_knob(field, ids):
    for f in (field, field[:-4] if field.endswith("_set") else field):
        if "KN_" + f.upper() in ids:
            return "KN_" + f.upper()
    raise AssertionError("RouteEnv field %s is not named after a switch" % field)


def route_rules():
    """{rule: set of KN_... its answer depends on}, rules called by a rule included."""
    ids = knob_ids()
    text = re.sub(r"//[^\n]*", "", open(os.path.join(_SRC, "route_host.h")).read())
    fields = set(re.findall(r"\b(\w+)(?= = [^;,]*[;,])", re.search(r"struct RouteEnv \{(.*?)\n\};", text, flags=re.S).group(1)))
    direct, calls = {}, {}
    for chunk in re.split(r"^inline ", text, flags=re.M)[1:]:
        name = re.match(r"[\w:<> ]*?(\w+)\(", chunk).group(1)
        read = set(re.findall(r"\be\.(\w+)", chunk))
        assert read <= fields, (name, read - fields)
        direct[name] = {_field_to_knob(f, ids) for f in read}
        calls[name] = set(re.findall(r"\b(route_\w+)\(", chunk)) - {name}
    assert direct["route_env"] == {_field_to_knob(f, ids) for f in fields}, "route_env fills every field of RouteEnv"

    def closure(name, seen):
        out = set(direct.get(name, ()))
        for c in calls.get(name, ()):
            if c not in seen:
                out |= closure(c, seen | {c})
        return out
    return {name: closure(name, {name}) for name in direct if name != "route_env"}


def switches_read(source_text, table_names):
    """Names (ISLE_...) of the switches the given source text reads."""
    ids = knob_ids()
    assert len(ids) == len(table_names), "knobs.h IsleKnob and isle_hip_switch_info disagree"
    rules = route_rules()
    used = set(re.findall(r"\bknob(?:_on)?\((KN_[A-Z0-9_]+)\)", source_text))
    used |= {_field_to_knob(f, ids) for f in re.findall(r"\broute\.(\w+)", source_text)}
    for r in set(re.findall(r"\b(route_\w+)\(", source_text)) - {"route_env"}:
        assert r in rules, "%s is not a rule of route_host.h" % r
        used |= rules[r]
    return {table_names[ids.index(k)] for k in used}
