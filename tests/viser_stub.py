"""A recording stand-in for the `viser` package, enough for the reference's `start_visualization` to run headless
(tools/make_golden_scene.py installs it as `viser` / `viser.transforms`): scene nodes that keep `points` / `colors` / `visible`, GUI
handles with `value` and callable `on_update` / `on_click`, and a fake client that captures `send_file_download`.

Assigning `handle.value` calls the handle's update callbacks, as the real GUI does when the user moves a control -- also when the
value stays the same, so that a generator can re-run a handler on purpose."""
import contextlib
import types


class Node:
    def __init__(self, name, **kw):
        self.name = name
        self.visible = kw.pop("visible", True)
        for k, v in kw.items():
            setattr(self, k, v)


class Event:
    def __init__(self, client=None):
        self.client = client


class Handle:
    def __init__(self, label, value=None):
        self.label = label
        self._value = value
        self.disabled = False
        self._update, self._click = [], []
        self.client = None   # handed to click events

    @property
    def value(self):
        return self._value

    @value.setter
    def value(self, v):
        self._value = v
        for f in list(self._update):
            f(Event(self.client))

    def on_update(self, f):
        self._update.append(f)
        return f

    def on_click(self, f):
        self._click.append(f)
        return f

    def click(self, client=None):
        for f in list(self._click):
            f(Event(client))


class Client:
    """captures what the server sends for download"""

    def __init__(self):
        self.downloads = []
        self.camera = types.SimpleNamespace(position=None, look_at=None)

    def send_file_download(self, name, data):
        self.downloads.append((name, bytes(data)))

    def atomic(self):
        return contextlib.nullcontext()

    def flush(self):
        pass


class Gui:
    def __init__(self):
        self.handles = {}

    def set_panel_label(self, *a, **k):
        pass

    def configure_theme(self, *a, **k):
        pass

    def add_folder(self, *a, **k):
        return contextlib.nullcontext()

    def _add(self, label, value=None):
        h = self.handles[label] = Handle(label, value)
        return h

    def add_slider(self, label, min=None, max=None, step=None, initial_value=None, **k):
        return self._add(label, initial_value)

    def add_checkbox(self, label, initial_value=False, **k):
        return self._add(label, initial_value)

    def add_button(self, label, **k):
        return self._add(label)

    def add_button_group(self, label, options=(), **k):
        return self._add(label, options[0] if options else None)


class SceneApi:
    def __init__(self):
        self.nodes = {}
        self.world_axes = types.SimpleNamespace(visible=True)

    def set_up_direction(self, *a, **k):
        pass

    def _add(self, name, **kw):
        n = self.nodes[name] = Node(name, **kw)
        return n

    def add_frame(self, name, **kw):
        return self._add(name, **kw)

    def add_point_cloud(self, name, points=None, colors=None, **kw):
        return self._add(name, points=points, colors=colors, **kw)

    def add_camera_frustum(self, name, **kw):
        return self._add(name, **kw)


class ViserServer:
    last = None   # the most recent instance: the generator reads its handles and nodes

    def __init__(self, *a, **k):
        self.gui = Gui()
        self.scene = SceneApi()
        ViserServer.last = self

    def on_client_connect(self, f):
        return f

    def atomic(self):
        return contextlib.nullcontext()

    def flush(self):
        pass

    def request_share_url(self):
        return None


class _SO3:
    def __init__(self, m):
        self.wxyz = (1.0, 0.0, 0.0, 0.0)

    @classmethod
    def from_matrix(cls, m):
        return cls(m)


def modules():
    """(viser, viser.transforms) as module objects for sys.modules"""
    v = types.ModuleType("viser")
    v.__path__ = []
    v.ViserServer, v.ClientHandle, v.GuiEvent = ViserServer, Client, Event
    t = types.ModuleType("viser.transforms")
    t.SO3 = _SO3
    v.transforms = t
    return v, t
