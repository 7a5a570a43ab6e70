"""Scenes for the integrator tests (test_integrator_host.py on the CPU, test_gpu_integrator.py on the
device): several refractive media of different eta and Kt, overlapping, at every depth the
frame stack admits.  TEST INFRASTRUCTURE (may use the oracle).

trace_sample (csrc/rt_kernels.hip) restates the reference's propagate_ray (scene.cu:92-188) rule
for rule: one Isect shared by a whole sample, REFLECT / REFRACT reading the material of whatever
was hit last, eta from the frame's own last_mat, time^Kt from the material hit on the way out,
in_obj inherited by reflection children, hit point and normal saved with a suspended frame, the
shadow loop through transmissive hits (light.cu:29-61).  With one refractive material those
rules cannot be told apart; these scenes have several, and the oracle's census
(Oracle.render(census=True)) counts how often each rule decided a frame.

Builders take any builder object (twin.Twin, a product scene or an oracle scene alone).

  media         32 unit cubes of five materials on a 4 x 4 x 2 lattice 0.8 apart (neighbours overlap;
                the upper layer 0.05 along x and 0.7 up), material (i + 2 j + 3 l) % 5:
                  0  Kr + Kt (.5, .6, .7, 1), Ks, alpha 4, eta 1.5
                  1  Kr + Kt (.9, .3, 0, 1), eta 0.8 (rarer than air: total internal reflection on entering)
                  2  Kt (1, .8, .6, 1), Ks, alpha 6, eta 1.0, no Kr
                  3  a mirror
                  4  opaque
                Rows j >= 2 stand 0.3 further along z: a slit about 0.05 to 0.1 wide between rows 1 and 2,
                whose facing walls both reflect in column i = 1 (both layers) and i = 3 (upper layer).
                A frame stack fills only by consecutive reflections (a refraction costs a level of
                depth without a push), and the outside of a field without a gap offers two or three:
                rays that enter the slit bounce between its walls `depth` times and more.
                A point light above, a directional light, and a point light inside the slit
                (shadow hits beyond the light).  Every cube is moved by its own multiple of 2^-9
                per axis (at most 31 / 512), so that no two cubes share a face plane: two
                coincident faces tie on the hit time, and which of them a traversal reports is its
                visiting order, not the integrator under test.
  media_kt_gt1  media with material 0's Kt = (.5, 1.25, .7, 1): a channel above 1 turns the unlit
                skip off on a refractive scene (shade_shortcuts, rt_plan.h).
  two_slabs     two separate refractive cubes (eta 1.5 and 0.8, different Kt, no Kr) in a row in front of
                the camera over an opaque floor: every REFRACT step follows its own frame's hit, so
                the Isect's material is the frame's last_mat throughout.  The control: a wrong frame
                here can be reasoned about by hand.
"""
import numpy as np

SIZE = (48, 32)
SCENES = ("media", "media_kt_gt1", "two_slabs")
DOWN45 = (0.3826834, 0.0, 0.0, 0.9238795)        # 45 degrees about x: forward (0, 0, 1) turns down
FOV, UNIT = 60.0, 100.0
DIST_ATTEN, AMBIENCE = (0.1, 0.05, 0.01), (0.3, 0.3, 0.3, 1.0)
LIGHT_INSIDE = (0.1, 0.35, 0.18)
KT_GT1 = (0.5, 1.25, 0.7, 1.0)
SLIT = 0.3       # rows j >= 2 stand this much further along z: a slit about 0.1 wide between rows 1 and 2


def material(Ke=(0, 0, 0, 0), Ka=(0, 0, 0, 0), Kd=(0, 0, 0, 0), Ks=(0, 0, 0, 0), Kt=(0, 0, 0, 0), Kr=(0, 0, 0, 0),
             alpha=0.0, eta=1.0):
    """material26 (rt_amd.h): Ke, Ka, Kd, Ks, Kt, Kr (4 each), alpha, eta."""
    return np.array(list(Ke) + list(Ka) + list(Kd) + list(Ks) + list(Kt) + list(Kr) + [alpha, eta], np.float32)


def media_materials(kt0=(0.5, 0.6, 0.7, 1.0)):
    ka = (0.1, 0.1, 0.1, 1)
    return [material(Ka=ka, Kd=(0.2, 0.2, 0.6, 1), Ks=(0.3, 0.3, 0.3, 1), Kt=kt0, Kr=(0.4, 0.4, 0.4, 1), alpha=4.0, eta=1.5),
            material(Ka=ka, Kd=(0.5, 0.2, 0.2, 1), Kt=(0.9, 0.3, 0.0, 1), Kr=(0.3, 0.3, 0.3, 1), eta=0.8),
            material(Ka=ka, Kd=(0.2, 0.5, 0.2, 1), Ks=(0.8, 0.8, 0.8, 1), Kt=(1.0, 0.8, 0.6, 1), alpha=6.0, eta=1.0),
            material(Ka=(0.05, 0.05, 0.05, 1), Kd=(0.3, 0.3, 0.3, 1), Kr=(0.7, 0.7, 0.7, 1)),
            material(Ka=ka, Kd=(0.6, 0.3, 0.1, 1))]


def media_cubes():
    """[(material index, centre)] of the 32 cubes; centres are float32-exact sums."""
    out = []
    for l in range(2):
        for j in range(4):
            for i in range(4):
                k = i + 4 * j + 16 * l
                # a different multiple of 2^-9 per cube on every axis (5 k + c mod 32 is a bijection of k)
                off = [((5 * k + 11 * a) % 32) / 512.0 for a in range(3)]
                c = (0.8 * (i - 1.5) + 0.05 * l + off[0], 0.7 * l + off[1], 0.8 * (j - 1.5) + (SLIT if j >= 2 else 0.0) + off[2])
                out.append(((i + 2 * j + 3 * l) % 5, tuple(float(np.float32(x)) for x in c)))
    return out


def face_planes(cubes, scale=1.0):
    """Per axis, the face-plane coordinates of axis-aligned cubes at float32 centres, as the instance
    transform sees them (centre -+ scale / 2 in float32)."""
    c = np.array([p for _, p in cubes], np.float32)
    h = np.float32(0.5 * scale)
    return [np.concatenate([c[:, a] - h, c[:, a] + h]) for a in range(3)]


# name -> (camera position, orientation).  "above": the kernel recipes' camera, looking 45 degrees down; it sees into
# the slit.  "inside": within the corner cube (0, 0, 0), material 0, clear of its neighbours, looking along -x at its
# free face -- the reference starts a sample with in_obj = false wherever the camera is.  "sky": lower and nearer,
# 27 degrees down: the slit in the lower rows, sky over the far edge of the field in the upper ones
MEDIA_POSES = {
    "above": ((0.1, 4.5, -4.2), DOWN45),
    "inside": ((-1.25, -0.1, -1.3), (0.0, -0.7071068, 0.0, 0.7071068)),
    "sky": ((0.1, 2.4, -1.4), (0.2334454, 0.0, 0.0, 0.9723699)),
}
INSIDE_CUBE = 0          # media_cubes() index of the cube the "inside" camera sits in


def build_media(b, size=SIZE, depth=9, kt0=(0.5, 0.6, 0.7, 1.0)):
    meshes = [b.build_cube(1.0, m) for m in media_materials(kt0)]
    for mat, pos in media_cubes():
        b.set_trans(b.add_trans(meshes[mat]), pos=pos)
    b.add_point_light((0.5, 6.0, -2.0), (1.0, 1.0, 1.0, 1.0))
    b.add_point_light(LIGHT_INSIDE, (0.8, 0.8, 0.6, 1.0))
    b.add_directional_light((0.3, -1.0, 0.8), (0.9, 0.8, 0.7, 1.0))
    pos, quat = MEDIA_POSES["above"]
    b.finish(size[0], size[1], FOV, UNIT, cam_pos=pos, cam_quat=quat, dist_atten=DIST_ATTEN, ambience=AMBIENCE,
             depth=depth)


SLABS = (((0.0, 0.1, 0.0), 1.5, (0.5, 0.6, 0.7, 1.0)), ((0.15, 0.2, 1.7), 0.8, (0.9, 0.3, 0.2, 1.0)))
SLABS_CAMERA = ((0.1, 1.6, -3.2), (0.1950903, 0.0, 0.0, 0.9807853))     # 22.5 degrees down, along the row


def build_two_slabs(b, size=SIZE, depth=9):
    ka = (0.1, 0.1, 0.1, 1)
    for k, (pos, eta, kt) in enumerate(SLABS):
        m = material(Ka=ka, Kd=(0.2, 0.2 + 0.3 * k, 0.6 - 0.3 * k, 1), Ks=(0.3, 0.3, 0.3, 1), Kt=kt, alpha=4.0, eta=eta)
        b.set_trans(b.add_trans(b.build_cube(1.0, m)), pos=pos)
    floor = b.build_cube(8.0, material(Ka=ka, Kd=(0.6, 0.5, 0.3, 1), Ks=(0.2, 0.2, 0.2, 1), alpha=8.0))
    b.set_trans(b.add_trans(floor), pos=(0.0, -4.7, 1.0))        # top at y = -0.7, under both slabs
    b.add_point_light((0.3, 3.0, -2.5), (1.0, 1.0, 1.0, 1.0))    # its shadow rays from the floor cross both slabs
    b.add_directional_light((0.0, -0.5, 1.0), (0.9, 0.8, 0.7, 1.0))
    pos, quat = SLABS_CAMERA
    b.finish(size[0], size[1], FOV, UNIT, cam_pos=pos, cam_quat=quat, dist_atten=DIST_ATTEN, ambience=AMBIENCE,
             depth=depth)


def build(b, name, size=SIZE, depth=9):
    if name == "media":
        build_media(b, size, depth)
    elif name == "media_kt_gt1":
        build_media(b, size, depth, kt0=KT_GT1)
    else:
        assert name == "two_slabs", name
        build_two_slabs(b, size, depth)


def poses(name):
    """{pose name: (position, orientation)} of a scene, its own camera first."""
    return dict(MEDIA_POSES) if name.startswith("media") else {"own": SLABS_CAMERA}


def census_row(c):
    """A census as one line, in oracle_lib.CENSUS order."""
    return " ".join("%s=%d" % kv for kv in c.items())
