"""CPU: the contact-regime atlas (tests/contact_atlas.py) certifies itself.

Each class is checked to hold the regime its name says, with the collider of
the independent model (``mjmodel_np.contacts``: every wall box, no roles), so
that tests/test_contact_atlas_gpu.py cannot pass by being empty; and the C
oracle is held to the enumeration model on the classes the model covers
(``mjmodel_np`` refuses a centre inside a wall box, so in_wall_cell and
off_map are oracle-only: finite outputs).
"""

import numpy as np
import pytest

import contact_atlas as ca
from oracle import locomaze as orc
from test_contact_pin import TOL_MODEL

BAND_WIDTH = 1e-3  # solimp width: |dist| below it is the impedance band


def _oracle(maze, q):
    return orc.physics(maze, q, np.zeros_like(q))


def _dists(maze, q):
    """Per state the sorted wall-contact distances."""
    return [sorted(d for d, _, _ in ca.wall_contacts(maze, x)) for x in q]


@pytest.mark.parametrize('maze', ca.MAZES)
def test_every_class_is_present(maze):
    at = ca.atlas(maze)
    assert tuple(at) == ca.CLASSES
    for label, q in at.items():
        assert q.ndim == 2 and q.shape[1] == 2 and q.dtype == np.float64, label
        assert len(q) > 0 or (label == 'in_wall_corner' and maze not in ca.IN_WALL_CORNER_MAZES), label
        assert np.isfinite(q).all(), label
        assert np.array_equal(q, ca.states(maze, label)), label  # deterministic
    S = ca.sites(maze)
    for kind, orientations in (('face', 4), ('outer', 4), ('inner', 4), ('on_edge', 8)):
        assert len({s[2:] for s in S[kind]}) == orientations, kind
    assert len({s[2:] for s in S['wall_corner']}) == (4 if maze in ca.IN_WALL_CORNER_MAZES else 0)
    assert len(ca.IN_WALL_CORNER_MAZES) >= 2


@pytest.mark.parametrize('maze', ca.MAZES)
def test_face_is_one_face_contact_off_axis(maze):
    q = ca.face(maze)
    depths = []
    for x in q:
        cons = ca.wall_contacts(maze, x)
        assert len(cons) == 1
        n = cons[0][1][0, :2]
        assert sorted(np.abs(n).tolist()) == [0.0, 1.0]
        depths.append(-cons[0][0])
        cell = np.round((x + ca.OFFSET) / ca.UNIT) * ca.UNIT - ca.OFFSET
        assert abs((x - cell) @ np.array([n[1], n[0]])) >= 0.05  # tangential offset
    depths = np.array(depths).reshape(-1, len(ca.BAND + ca.DEEP))
    assert np.abs(depths - np.array(ca.BAND + ca.DEEP)).max() <= 1e-13
    assert len(depths) >= 4


@pytest.mark.parametrize('maze', ca.MAZES)
def test_outer_corner_is_one_diagonal_contact(maze):
    q = ca.outer_corner(maze)
    band = 0
    quadrants = set()
    for x in q:
        cons = ca.wall_contacts(maze, x)
        assert len(cons) == 1
        dist, fr, _ = cons[0]
        n = fr[0, :2]
        assert np.abs(n).min() > 0.02  # neither face's normal
        quadrants.add((np.sign(n[0]), np.sign(n[1])))
        band += abs(dist) < BAND_WIDTH
    assert band >= 15
    assert len(quadrants) == 4  # all four orientations
    d = np.array([-c[0][0] for c in map(lambda x: ca.wall_contacts(maze, x), q)]).reshape(4, -1, 3)
    assert np.abs(d - np.array(ca.BAND + ca.DEEP)[None, :, None]).max() <= 1e-13


@pytest.mark.parametrize('maze', ca.MAZES)
def test_inner_corner_band_beside_deep_and_three_walls(maze):
    q = ca.inner_corner(maze)
    dd = _dists(maze, q)
    assert min(len(d) for d in dd) >= 2

    def beside(d):
        return any(abs(a) < BAND_WIDTH for a in d) and any(abs(a) >= min(ca.DEEP) for a in d)

    mixed = np.array([beside(d) for d in dd])
    three = np.array([len(d) == 3 for d in dd])
    assert mixed.sum() >= 15 and three.sum() >= 15
    assert (np.array([len(d) for d in dd]) <= 3).all()
    # the part that goes to the model keeps the mixed minimum in every maze,
    # and the three-wall one over the mazes (test_model_subsets_keep_the_minima)
    sub = ca.model_subset(maze, 'inner_corner')
    assert mixed[sub].sum() >= 15
    assert three[sub].sum() == ca.MODEL_CAP3['inner_corner']


def test_model_subsets_keep_the_minima():
    three = 0
    for maze in ca.MAZES:
        for label in ca.MODEL_CLASSES:
            sub = ca.model_subset(maze, label)
            q = ca.states(maze, label)[sub]
            nw = np.array([len(ca.wall_contacts(maze, x)) for x in q])
            assert len(sub) == len(set(sub.tolist())) > 0 and (nw >= 1).all(), (maze, label)
            three += int((nw >= 3).sum())
    assert 15 <= three <= 24  # the enumeration takes 0.2-1 s per three-wall state


@pytest.mark.parametrize('maze', ca.MAZES)
def test_edge_wall_end_straddles_the_cell_edge(maze):
    q = ca.edge_wall_end(maze).reshape(-1, len(ca.EDGE_PEN), len(ca.EDGE_E), 2)
    assert q.shape[0] == 8  # four orientations, the edge on either axis
    for g, grp in enumerate(q):
        axis = g % 2  # axis 0: x holds the penetration, y crosses the edge
        for p, pen in enumerate(ca.EDGE_PEN):
            for k, e in enumerate(ca.EDGE_E):
                x = grp[p, k]
                cons = ca.wall_contacts(maze, x)
                assert len(cons) == 1
                n = np.abs(cons[0][1][0, :2])
                lo = (x[1 - axis] + ca.OFFSET + ca.HALF) % ca.UNIT  # offset from the cell edge
                if e == 0.0:
                    assert lo == 0.0  # exactly on the edge
                if e < 0.0:
                    assert n.min() > 0.0  # the box corner: a diagonal normal
                    assert abs(cons[0][0] - (np.hypot(ca.RADIUS - pen, e) - ca.RADIUS)) <= 1e-13
                else:
                    assert n[axis] == 1.0 and n[1 - axis] == 0.0  # the face
                    assert abs(-cons[0][0] - pen) <= 1e-13


@pytest.mark.parametrize('maze', ca.MAZES)
def test_on_edge_face_is_exactly_on_the_edge(maze):
    q = ca.on_edge_face(maze)
    kinds = set()
    for x in q:
        # the kernel's and the oracle's cell of the centre, and the offset in it
        cell = np.floor((x + ca.OFFSET + 0.5 * ca.UNIT) / ca.UNIT)
        l = x - (cell * ca.UNIT - ca.OFFSET)
        on = np.abs(l) == ca.HALF
        assert on.sum() == 1
        cons = ca.wall_contacts(maze, x)
        assert 1 <= len(cons) <= 2
        for dist, fr, _ in cons:
            n = fr[0, :2]
            assert abs(n[on.argmax()]) == 0.0 and abs(n[1 - on.argmax()]) == 1.0  # a face on the other axis
            kinds.add((int(on.argmax()), float(n[1 - on.argmax()])))
    assert len(kinds) == 4  # both axes, both signs
    assert len(q) == 8 * len(ca.EDGE_PEN)


@pytest.mark.parametrize('maze', ca.MAZES)
def test_rest_holds_resting_contacts(maze):
    q = ca.rest(maze)
    press = ca.rest_press(maze)
    assert q.shape == press.shape and len(q) % (3 * len(ca.REST_STEPS)) == 0
    mag = np.linalg.norm(press, axis=1)
    assert np.abs(mag[:, None] - np.array(ca.REST_PRESS)).min(1).max() <= 1e-15 and max(ca.REST_PRESS) <= 0.01
    _, flag = _oracle(maze, q)
    pen = np.array([min([abs(d) for d in dd], default=np.inf) for dd in _dists(maze, q)])
    assert ((pen < 1e-9) & (flag == 1)).sum() >= 20
    # the band from its bottom (a few ulp) to its top, not its floor alone
    assert ((pen >= 1e-9) & (pen < 1e-5)).sum() >= 20 and ((pen >= 1e-5) & (pen < BAND_WIDTH)).sum() >= 20
    sub = ca.model_subset(maze, 'rest')
    assert (pen[sub] < 1e-9).sum() >= 5 and (pen[sub] < BAND_WIDTH).sum() >= 20


@pytest.mark.parametrize('maze', ca.MAZES)
@pytest.mark.parametrize('label', ['flag_face', 'flag_corner'])
def test_flag_classes_hold_both_flag_values(maze, label):
    q = ca.states(maze, label)
    assert len(q) == len(ca.FLAG_K) * ca.FLAG_PER_K
    out, flag = _oracle(maze, q)
    assert 0.2 <= flag.mean() <= 0.8
    assert np.array_equal(out[flag == 0], q[flag == 0])
    # both values well inside the ulp range, not only at its ends
    by_k = flag.reshape(len(ca.FLAG_K), -1).mean(1)
    assert by_k[:3].mean() > 0.5 > by_k[-3:].mean()


@pytest.mark.parametrize('maze', ca.MAZES)
@pytest.mark.parametrize('label', ca.MODEL_CLASSES)
def test_oracle_matches_model_on_class(maze, label):
    sub = ca.model_subset(maze, label)
    q = ca.states(maze, label)[sub]
    got, flag = _oracle(maze, q)
    assert flag.all()
    err = np.abs(got - ca.model_answers(maze, label)).max()
    assert err <= TOL_MODEL, err


@pytest.mark.parametrize('maze', ca.MAZES)
def test_in_wall_corner_touches_four_boxes(maze):
    """The generic collider's four-contact regime, by geometry: the centre in
    a wall cell, at least 1.3 from its centre on both axes, within the radius
    of the corner, and exactly four wall boxes within the radius; every depth
    of BAND and DEEP in all four orientations; the oracle's output finite."""
    mp = ca.maze_map(maze)
    q = ca.in_wall_corner(maze)
    if maze not in ca.IN_WALL_CORNER_MAZES:  # no 2 x 2 block of wall cells in this map
        block = mp[:-1, :-1] & mp[1:, :-1] & mp[:-1, 1:] & mp[1:, 1:]
        assert not block.any() and q.shape == (0, 2)
        return
    nd = len(ca.BAND + ca.DEEP)
    assert len(q) == 4 * nd * 4 and len(q) >= 100
    cell = np.floor((q + ca.OFFSET + 0.5 * ca.UNIT) / ca.UNIT).astype(int)
    assert (mp[cell[:, 1], cell[:, 0]] == 1).all()
    l = q - (cell * ca.UNIT - ca.OFFSET)
    assert (np.abs(l) >= ca.HALF - ca.RADIUS).all() and (np.abs(l) < ca.HALF).all()
    rc = np.hypot(*(ca.HALF - np.abs(l)).T)
    want = ca.RADIUS - np.repeat(np.tile(ca.BAND + ca.DEEP, 4), 4)
    assert np.abs(rc - want).max() <= 1e-13 and (rc <= ca.RADIUS).all()
    assert (rc[want > ca.RADIUS - 1e-3] > ca.RADIUS - 1e-3).sum() >= 15  # the diagonal slot inside the band
    assert len({(s0, s1) for s0, s1 in np.sign(l).tolist()}) == 4
    assert [ca.touching_boxes(maze, x) for x in q] == [4] * len(q)
    out, flag = _oracle(maze, q)
    assert np.isfinite(out).all() and flag.all()
    # the random in_wall_cell draw holds such states only by luck
    print(maze, 'in_wall_cell states with four boxes:', sum(ca.touching_boxes(maze, x) == 4 for x in ca.in_wall_cell(maze)))


@pytest.mark.parametrize('maze', ca.MAZES)
def test_oracle_only_classes_are_finite(maze):
    mp = ca.maze_map(maze)
    H, W = mp.shape
    q = ca.in_wall_cell(maze)
    cell = np.floor((q + ca.OFFSET + 0.5 * ca.UNIT) / ca.UNIT).astype(int)
    assert (mp[cell[:, 1], cell[:, 0]] == 1).all()
    out, flag = _oracle(maze, q)
    assert np.isfinite(out).all() and flag.all()
    q = ca.off_map(maze)
    cell = np.floor((q + ca.OFFSET + 0.5 * ca.UNIT) / ca.UNIT)
    assert ((cell[:, 0] < 0) | (cell[:, 0] >= W) | (cell[:, 1] < 0) | (cell[:, 1] >= H)).all()
    out, flag = _oracle(maze, q)
    assert np.isfinite(out).all()
    assert flag.sum() >= 10 and (flag == 0).sum() >= 10  # within the radius of the outer wall, and beyond it
    assert np.array_equal(out[flag == 0], q[flag == 0])
