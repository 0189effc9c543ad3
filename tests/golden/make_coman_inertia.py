"""Generates tests/golden/coman_inertia.json from the reference's robot description
(/root/reference/tests/robots/coman_floating_base/coman_floating_base.urdf).  Run in the build container only.

The fixture is DATA: for every moving joint of tests/golden/coman_tree.json (same order) the rotational inertia tensor
[Ixx Ixy Ixz Iyy Iyz Izz] of everything rigidly attached to it -- links behind fixed joints merged into their moving ancestor
with the parallel-axis theorem -- about the MERGED centre of mass, axes of the joint frame (osot_dyn_desc.inertia).  The
traversal is that of make_coman_tree.py; merged masses and centres of mass must reproduce coman_tree.json to 1e-12."""
import json, os
import xml.etree.ElementTree as ET
import numpy as np

URDF = "/root/reference/tests/robots/coman_floating_base/coman_floating_base.urdf"
HERE = os.path.dirname(os.path.abspath(__file__))
TREE = os.path.join(HERE, "coman_tree.json")
OUT = os.path.join(HERE, "coman_inertia.json")


def rpy(r, p, y):
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


def vec(s, d=(0.0, 0.0, 0.0)):
    return np.array([float(v) for v in s.split()]) if s else np.array(d, dtype=float)


root = ET.parse(URDF).getroot()
links = {}
for l in root.findall("link"):
    m, c, Rc, I = 0.0, np.zeros(3), np.eye(3), np.zeros((3, 3))
    ine = l.find("inertial")
    if ine is not None:
        m = float(ine.find("mass").get("value"))
        o = ine.find("origin")
        if o is not None:
            c = vec(o.get("xyz")); Rc = rpy(*vec(o.get("rpy")))
        t = ine.find("inertia")
        if t is not None:
            g = lambda k: float(t.get(k, "0"))
            I = np.array([[g("ixx"), g("ixy"), g("ixz")], [g("ixy"), g("iyy"), g("iyz")], [g("ixz"), g("iyz"), g("izz")]])
    links[l.get("name")] = (m, c, Rc @ I @ Rc.T)          # tensor about the link's centre of mass, axes of the link frame
children = {}
for j in root.findall("joint"):
    o = j.find("origin")
    xyz = vec(o.get("xyz")) if o is not None and o.get("xyz") else np.zeros(3)
    R = rpy(*vec(o.get("rpy"))) if o is not None and o.get("rpy") else np.eye(3)
    children.setdefault(j.find("parent").get("link"), []).append(
        dict(name=j.get("name"), type=j.get("type"), child=j.find("child").get("link"), R=R, p=xyz))

bodies = []      # per moving joint: the (mass, centre of mass, tensor about it) of every attached link, in the joint frame


def attach(link, jidx, R, p):
    m, c, I = links[link]
    bodies[jidx].append((m, R @ c + p, R @ I @ R.T))
    for ch in children.get(link, []):
        Rj, pj = R @ ch["R"], R @ ch["p"] + p
        if ch["type"] == "fixed":
            attach(ch["child"], jidx, Rj, pj)
        elif ch["type"] in ("revolute", "continuous", "prismatic"):
            bodies.append([])
            attach(ch["child"], len(bodies) - 1, np.eye(3), np.zeros(3))
        else:
            raise SystemExit("unsupported joint type " + ch["type"])


fl = [c for c in children["world"] if c["type"] == "floating"]
assert len(fl) == 1
for _ in range(6):
    bodies.append([])
attach(fl[0]["child"], 5, np.eye(3), np.zeros(3))

tree = json.load(open(TREE))
assert len(bodies) == tree["n"], (len(bodies), tree["n"])
rows = []
for j, parts in enumerate(bodies):
    m = sum(b[0] for b in parts)
    c = sum((b[0] * b[1] for b in parts), np.zeros(3)) / m if m > 0 else np.zeros(3)
    I = np.zeros((3, 3))
    for mb, cb, Ib in parts:
        d = cb - c
        I += Ib + mb * (d @ d * np.eye(3) - np.outer(d, d))      # parallel axes
    J = tree["joints"][j]
    assert abs(m - J["mass"]) <= 1e-12 and np.abs(c - np.array(J["com"])).max() <= 1e-12, (j, m, J["mass"], c, J["com"])
    w = np.linalg.eigvalsh(I)
    assert w.min() >= -1e-15 and w[0] + w[1] >= w[2] - 1e-12 * max(w[2], 1e-300), (j, w)
    rows.append([float(I[0, 0]), float(I[0, 1]), float(I[0, 2]), float(I[1, 1]), float(I[1, 2]), float(I[2, 2])])
doc = {"source": "tests/robots/coman_floating_base/coman_floating_base.urdf (ADVRHumanoids/OpenSoT @2024-10-24), reduced by tests/golden/make_coman_inertia.py",
       "n": len(rows), "names": [J["name"] for J in tree["joints"]],
       "inertia": rows}
json.dump(doc, open(OUT, "w"), indent=0)
print(len(rows), "tensors ->", OUT, os.path.getsize(OUT), "bytes")
