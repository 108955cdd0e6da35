"""Small synthetic URDFs for the dynamics known-answer tests (test infrastructure).

two_link(): planar 2R arm (joints about y, links along x) whose mass matrix,
gravity and Coriolis terms have the textbook closed forms (Spong, Robot
Modeling and Control, §7.4).  rank_deficient(): a 3R chain whose last link has
no <inertial>, so M(q) has a zero row/column and PinvCOD must return the
rank-2 pseudo-inverse (robot_data.cpp:118).  swing_arm(): a 3R chain whose
M(q) is well conditioned except where its long link lies on joint 1's axis,
where it loses a mode (below)."""
import os

import numpy as np

TWO_LINK = dict(m1=1.7, m2=0.9, l1=0.55, lc1=0.3, lc2=0.21, I1=0.031, I2=0.017)


def _inertial(m, com, iyy, ixx=None, izz=None):
    ixx = iyy if ixx is None else ixx
    izz = iyy if izz is None else izz
    return ('<inertial><origin xyz="%r %r %r" rpy="0 0 0"/><mass value="%r"/>'
            '<inertia ixx="%r" ixy="0" ixz="0" iyy="%r" iyz="0" izz="%r"/></inertial>'
            % (com[0], com[1], com[2], m, ixx, iyy, izz))


def two_link(dirpath):
    p = TWO_LINK
    urdf = f"""<?xml version="1.0"?>
<robot name="two_link">
  <link name="base"/>
  <link name="link1">{_inertial(p['m1'], (p['lc1'], 0, 0), p['I1'])}</link>
  <link name="link2">{_inertial(p['m2'], (p['lc2'], 0, 0), p['I2'])}</link>
  <joint name="j1" type="revolute"><parent link="base"/><child link="link1"/>
    <origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="0 1 0"/><limit lower="-3" upper="3" velocity="2" effort="10"/></joint>
  <joint name="j2" type="revolute"><parent link="link1"/><child link="link2"/>
    <origin xyz="{p['l1']!r} 0 0" rpy="0 0 0"/><axis xyz="0 1 0"/><limit lower="-3" upper="3" velocity="2" effort="10"/></joint>
</robot>
"""
    path = os.path.join(dirpath, "two_link.urdf")
    with open(path, "w") as f:
        f.write(urdf)
    return path


def two_link_closed_form(q, qd, grav=9.81):
    p = TWO_LINK
    m1, m2, l1, lc1, lc2, I1, I2 = (p[k] for k in ("m1", "m2", "l1", "lc1", "lc2", "I1", "I2"))
    c2, s2 = np.cos(q[1]), np.sin(q[1])
    M = np.array([[m1 * lc1 ** 2 + I1 + m2 * (l1 ** 2 + lc2 ** 2 + 2 * l1 * lc2 * c2) + I2,
                   m2 * (lc2 ** 2 + l1 * lc2 * c2) + I2],
                  [m2 * (lc2 ** 2 + l1 * lc2 * c2) + I2, m2 * lc2 ** 2 + I2]])
    # rotation about +y tilts +x towards -z: height of a point at distance r is -r sin(angle)
    g = np.array([-(m1 * lc1 + m2 * l1) * grav * np.cos(q[0]) - m2 * lc2 * grav * np.cos(q[0] + q[1]),
                  -m2 * lc2 * grav * np.cos(q[0] + q[1])])
    h = m2 * l1 * lc2 * s2
    c = np.array([-h * (2 * qd[0] * qd[1] + qd[1] ** 2), h * qd[0] ** 2])
    return M, g, c


def rank_deficient(dirpath):
    urdf = f"""<?xml version="1.0"?>
<robot name="rank_deficient">
  <link name="base"/>
  <link name="a">{_inertial(1.2, (0.1, 0.0, 0.05), 0.02, 0.01, 0.015)}</link>
  <link name="b">{_inertial(0.8, (0.0, 0.12, 0.0), 0.01, 0.012, 0.008)}</link>
  <link name="c"/>
  <joint name="j1" type="revolute"><parent link="base"/><child link="a"/>
    <origin xyz="0 0 0.1" rpy="0 0 0"/><axis xyz="0 0 1"/><limit lower="-3" upper="3" velocity="2" effort="10"/></joint>
  <joint name="j2" type="revolute"><parent link="a"/><child link="b"/>
    <origin xyz="0.2 0 0" rpy="0 0.3 0"/><axis xyz="1 0 0"/><limit lower="-3" upper="3" velocity="2" effort="10"/></joint>
  <joint name="j3" type="revolute"><parent link="b"/><child link="c"/>
    <origin xyz="0 0.25 0" rpy="0 0 0"/><axis xyz="0 0 1"/><limit lower="-3" upper="3" velocity="2" effort="10"/></joint>
</robot>
"""
    path = os.path.join(dirpath, "rank_deficient.urdf")
    with open(path, "w") as f:
        f.write(urdf)
    return path


SWING = dict(m=5.0, L=0.8, rotor=2e-7)


def swing_arm(dirpath):
    """3R chain: joint 1 about z; joint 2 about y at the same point, carrying a
    long slender link (length L along its x) with a heavy mass m at the tip;
    joint 3 about that link's own x at the tip, carrying a compact body.  The
    tip mass swings on and off joint 1's axis with q[1]: at q[1] = +-pi/2 the
    link lies on the axis, joints 1 and 3 turn the same bodies about the same
    line, and what is left of M's smallest mode is the base rotor's inertia,
    6e-8 of the m L^2 = 3.2 that joint 2 always carries.  There PinvCOD drops
    the mode; a few degrees away M is certified full rank (condition ~1e3)."""
    p = SWING
    urdf = f"""<?xml version="1.0"?>
<robot name="swing_arm">
  <link name="base"/>
  <link name="a">{_inertial(0.3, (0.0, 0.0, 0.0), 1e-3, 1e-3, p['rotor'])}</link>
  <link name="b">{_inertial(p['m'], (p['L'], 0.0, 0.0), 2e-3, 1e-8, 2e-3)}</link>
  <link name="c">{_inertial(0.4, (0.0, 0.0, 0.0), 3e-3, 4e-3, 3e-3)}</link>
  <joint name="j1" type="revolute"><parent link="base"/><child link="a"/>
    <origin xyz="0 0 0.1" rpy="0 0 0"/><axis xyz="0 0 1"/><limit lower="-3" upper="3" velocity="2" effort="10"/></joint>
  <joint name="j2" type="revolute"><parent link="a"/><child link="b"/>
    <origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="0 1 0"/><limit lower="-3" upper="3" velocity="2" effort="10"/></joint>
  <joint name="j3" type="revolute"><parent link="b"/><child link="c"/>
    <origin xyz="{p['L']!r} 0 0" rpy="0 0 0"/><axis xyz="1 0 0"/><limit lower="-3" upper="3" velocity="2" effort="10"/></joint>
</robot>
"""
    path = os.path.join(dirpath, "swing_arm.urdf")
    with open(path, "w") as f:
        f.write(urdf)
    return path
