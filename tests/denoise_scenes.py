"""The three scenes of the denoiser tests.  A helper module: no tests live here, and nothing here needs the device."""
import numpy as np


def open_scene(w, h, mesh=True):
    """Floor, back wall and the emitter of the box only (plus a 1,280-triangle ball: not LDS-resident, so the 4-wide walk is
    available): the top and the sides of the frame see nothing."""
    import clive2_amd as c2
    from clive2_amd.load import get_materials, triangles_for_box
    from clive2_amd.meshes import icosphere
    keep = [t for t in triangles_for_box() if t.emitter or t.n[1] > 0.5 or t.n[2] > 0.5]
    specs = [dict(mesh=icosphere(3, radius=1.5), material=5, offset=np.array([0.5, 0.0, -1.0]))] if mesh else None
    return c2.create_scene(w, h, np.array([0, 1.5, 6]), np.array([0, 0, -1]), room=keep, materials=get_materials(),
                           file_specs=specs)


def glass(w, h):
    import clive2_amd as c2
    from clive2_amd.load import get_materials
    from clive2_amd.meshes import icosphere
    mats = get_materials()
    mats["alpha"][5] = 0.1
    v, f = icosphere(2, radius=2.0, center=(0.0, 1.0, 0.0))
    return c2.create_scene(w, h, np.array([0, 1.5, 6]), np.array([0, 0, -1]), file_specs=[dict(mesh=(v, f), material=5)],
                           materials=mats)


def cornell(w, h):
    import clive2_amd as c2
    return c2.create_scene_from_preset("empty", w, h)
