"""The policy headers (coloc_amd/host/*.hpp) compile in two worlds: stand-alone against the stand-in types of this
repository, and inside the reference tree (COLOC_HIP_WITH_OPENMVG) against the real openMVG / Eigen / OpenCV types -- which
are not installed here, so that branch cannot be compiled.  What CAN be checked without them: every name the headers use as a
member, method or qualified name is either one the reference's OWN sources use (tests/golden/reference_member_names.json,
tools/gen_reference_member_names.py) or is listed, with its justification, in INTEGRATION.md section 4c.  A member the
stand-ins invented (round 2: IntrinsicBase::bearing) fails here."""
import glob
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.sub(r'"(\\.|[^"\\])*"', '""', text)


def used_member_names():
    used = {}
    for f in sorted(glob.glob(os.path.join(ROOT, "coloc_amd", "host", "*.hpp"))):
        text = strip_comments(open(f).read())
        for m in re.finditer(r"(\b[A-Za-z_]\w*\s*)?(\.|->|::)\s*([A-Za-z_]\w*)", text):
            if (m.group(1) or "").strip() == "std":
                continue                                     # the C++ standard library is not under test
            used.setdefault(m.group(3), set()).add(os.path.basename(f))
    return used


def documented_exceptions():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("### 4c."):text.index("## 5.")]
    names = set()
    for row in re.findall(r"^\| (`[^|]*) \|", sec, flags=re.M):
        names |= set(re.findall(r"`([A-Za-z_]\w*)(?:\(\))?`", row))
    return names


def test_every_member_is_the_references_or_documented():
    ref = set(json.load(open(os.path.join(ROOT, "tests", "golden", "reference_member_names.json")))["names"])
    allowed = documented_exceptions()
    assert {"focal", "principal_point", "statePre", "statePost"} <= allowed
    used = used_member_names()
    assert len(used) > 80
    unknown = {n: sorted(fs) for n, fs in used.items() if n not in ref and n not in allowed}
    assert not unknown, "names used by the policy headers that neither the reference uses nor INTEGRATION.md 4c lists: %r" % unknown
    assert "bearing" not in used                              # the invented member of round 2 stays gone


HEADER_OF = {"detector": "HIPDetector.hpp", "matcher": "HIPMatcher.hpp", "localizer": "HIPLocalizer.hpp", "robustMatcher": "HIPRobustMatcher.hpp",
             "filter": "HIPPoseFilter.hpp", "covIntOptimizer": "HIPCovIntersection.hpp", "logger": "HIPPoseLog.hpp"}


def declared_members(header):
    """names a header declares as member functions or data members (anything followed by `(`, `=`, `;`, `{` or `[` outside comments)"""
    text = strip_comments(open(os.path.join(ROOT, "coloc_amd", "host", header)).read())
    return set(re.findall(r"\b([A-Za-z_]\w*)\s*(?=\(|=|;|\{|\[)", text))


def test_every_member_the_references_callers_use_is_declared():
    """The converse of the test above: whatever coloc.hpp / colocInterface.hpp / InterfaceDisk.hpp / InterfaceROS.hpp call on
    `detector.` / `matcher.` / `localizer.` / `robustMatcher.` / `filter.` / `covIntOptimizer.` / `logger.`
    (tests/golden/reference_policy_calls.json, tools/gen_reference_policy_calls.py) must be a member of the matching header here, or be
    listed with its reason in INTEGRATION.md 4c -- round 3 shipped HIPRobustMatcher without matchMaps (coloc.hpp:326, :443)."""
    calls = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_policy_calls.json")))["calls"]
    assert set(calls) == set(HEADER_OF) and "matchMaps" in calls["robustMatcher"] and "localizeImage" in calls["localizer"]
    allowed = documented_exceptions()
    missing = {}
    for obj, members in calls.items():
        have = declared_members(HEADER_OF[obj])
        lost = [m for m in members if m not in have and m not in allowed]
        if lost:
            missing[obj] = lost
    assert not missing, "members the reference's callers use that the HIP policy headers do not declare: %r" % missing


def test_reference_call_forms_are_the_ones_used():
    rm = strip_comments(open(os.path.join(ROOT, "coloc_amd", "host", "HIPRobustMatcher.hpp")).read())
    # bearing vectors the way RobustMatcher.hpp:159 asks for them
    assert re.search(r"\(\*intrinsics1\)\(x1\)", rm) and re.search(r"\(\*intrinsics2\)\(x2\)", rm)
    # the only partially assigned matrix of round 2 is now assigned in full
    assert re.search(r"W\(i, k\) = 0\.0", rm)
