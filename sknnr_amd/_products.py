"""The side products of one streamed call: what a stream computes beside its results and the call adds to the
user's objects afterwards -- neighbour usage, zonal statistics, the distance domain and the bootstrap's tallies.

:class:`StreamProducts` is the one place a product is wired into the streamed calls of ``_base.py``, for searched
and for replayed tiles alike, at four moments:

    check     ``check_*`` / ``bootstrap_request``: every refusal, before any device work
    open      ``open_keywords``: the product keywords of ``open_stream`` / ``open_replay``
    feed      ``next_tile`` / ``feed`` / ``end_of_tiles``: what a tile brings along (zone codes, the domain_out window)
    collect   ``collect`` reads the stream's accumulators before it is closed; ``commit`` adds them to the user's
              objects, only once the whole call has succeeded
"""

from __future__ import annotations

import numpy as np

from ._domain import DistanceDomain
from ._usage import NeighborUsage
from ._zonal import ZonalStats

_ZONES_SHORT = "zones ended before tiles: the call needs one array of zone codes per tile"
_ZONES_LONG = "tiles ended before zones: the call needs one array of zone codes per tile"


def normalize_zone_tile(zones, n):
    """The zone codes of one streamed tile of ``n`` pixels -- ``(n,)``, or ``(h, w)`` in the pixels' C order -- as a
    C-contiguous int32 ``(n,)`` array.  Any integer dtype is accepted; a value outside int32 is a ``ValueError``."""
    zones = np.asarray(zones)
    if zones.dtype.kind not in "iu":
        raise ValueError(f"zones must hold integer zone codes, got {zones.dtype}")
    if zones.size != n:
        raise ValueError(f"zones must hold one code per pixel of its tile ({n}), got {zones.size} (shape {zones.shape})")
    if zones.dtype != np.int32 and zones.size:
        info = np.iinfo(np.int32)
        if zones.min() < info.min or zones.max() > info.max:
            raise ValueError(f"zone codes must fit int32, got values in [{zones.min()}, {zones.max()}]")
    return np.ascontiguousarray(zones, dtype=np.int32).reshape(-1)


class StreamProducts:
    """``usage`` (a :class:`sknnr_amd.NeighborUsage`), ``zones`` / ``zonal`` (an iterable in lockstep with the tiles, a
    :class:`sknnr_amd.ZonalStats`), ``domain`` / ``domain_out`` / ``beyond`` (a :class:`sknnr_amd.DistanceDomain`, the
    uint8 plane that receives its codes, "nodata" to blank the predictions beyond its threshold) and ``bootstrap`` (a
    :class:`sknnr_amd.Bootstrap`; :meth:`bootstrap_request` makes its ``request``) of one streamed call.  ``est`` is the
    :class:`sknnr_amd._base.RawKNNRegressor` that streams.  The checks are separate methods because the calls interleave
    them with their other refusals; a replay, which learns ``k`` from its first tile, calls them without ``k`` first and
    :meth:`settle` then.  Falsy when the call has no product at all."""

    def __init__(self, usage=None, zones=None, zonal=None, domain=None, domain_out=None, beyond="keep", bootstrap=None):
        self.usage, self.zones, self.zonal, self.bootstrap = usage, zones, zonal, bootstrap
        self.domain, self.domain_out, self.beyond = domain, domain_out, beyond
        self.request = self._zonal_binding = self._tile_zones = None
        self._collected = {}

    def __bool__(self):
        return any(v is not None for v in (self.usage, self.zones, self.zonal, self.domain, self.domain_out,
                                           self.bootstrap)) or self.beyond != "keep"

    @property
    def blank(self) -> bool:
        return self.beyond == "nodata"

    # -- check ---------------------------------------------------------------------------------------
    def check_beyond(self) -> bool:
        if self.beyond not in ("keep", "nodata"):
            raise ValueError(f"beyond must be 'keep' or 'nodata', got {self.beyond!r}")
        return self.blank

    def check_usage(self, est, k=None, host_callable=False):
        """``k`` None: what can be checked before the number of neighbours is known."""
        if self.usage is None:
            return
        if host_callable:
            est._refuse_callable_weights("usage is")
        est._check_stream_supported("usage is")
        if not isinstance(self.usage, NeighborUsage):
            raise TypeError(f"usage must be a sknnr_amd.NeighborUsage, got {type(self.usage).__name__}")
        if k is not None:
            self.usage._check(est.n_samples_fit_, k)  # (a mismatch is refused before any device work)

    def check_domain(self, est, k=None, host_callable=False):
        """Every refusal of ``domain`` / ``domain_out`` / the mask; ``k`` None: all but the rank's."""
        domain, domain_out = self.domain, self.domain_out
        if domain is None:
            if domain_out is not None:
                raise ValueError("domain_out needs domain: the DistanceDomain whose codes it receives")
            if self.blank:
                raise ValueError("beyond='nodata' needs domain: a DistanceDomain with a threshold")
            return
        if not isinstance(domain, DistanceDomain):
            raise TypeError(f"domain must be a sknnr_amd.DistanceDomain, got {type(domain).__name__}")
        if host_callable:
            est._refuse_callable_weights("domain is")
        est._check_stream_supported("domain is")
        if k is not None and domain.rank > k:
            raise ValueError(f"domain.rank={domain.rank} is above n_neighbors={k}")
        if self.blank and domain.threshold is None:
            raise ValueError("beyond='nodata' needs a DistanceDomain with a threshold")
        if domain_out is not None and (not isinstance(domain_out, np.ndarray) or domain_out.dtype != np.uint8
                                       or domain_out.ndim != 1 or not domain_out.flags.c_contiguous
                                       or not domain_out.flags.writeable):
            raise ValueError("domain_out must be a writable C-contiguous uint8 (N_total,) array, one element per pixel")

    def check_zonal(self, est, n_planes, output, host_callable=False):
        """``output``: the typed output of the ``n_planes`` prediction planes (:func:`normalize_typed_output`).  Keeps the
        binding ``zonal`` gets when the call has come through."""
        zones, zonal = self.zones, self.zonal
        if zones is None and zonal is None:
            return
        if zones is None or zonal is None:
            raise ValueError("zones and zonal come together: the zone codes of every tile, and the ZonalStats they are "
                             "tallied into")
        if not isinstance(zonal, ZonalStats):
            raise TypeError(f"zonal must be a sknnr_amd.ZonalStats, got {type(zonal).__name__}")
        if host_callable:
            est._refuse_callable_weights("zonal is")
        est._check_stream_supported("zonal is")
        if not output or np.dtype(output["pred_dtype"]).kind not in "iu":
            raise NotImplementedError("zonal needs an integer out_dtype (int16, uint16, uint8 or int32): a float atomic "
                                      "sum is order-dependent, so zonal sums are taken over the stored integers of a "
                                      "typed output")
        self._zonal_binding = zonal._check(n_planes, output["pred_dtype"], output.get("scale"), output.get("offset"))
        self.zones = iter(zones)

    def settle(self, est, k):
        """What needs the number of neighbours, for a call that checked without it."""
        self.check_usage(est, k)
        self.check_domain(est, k)

    def bootstrap_request(self, est, statistic, outputs, *, return_neighbors=False, return_dataframe_index=False,
                          neighbors_out=None, index_dtype=None, distance_dtype=None, n_targets=None, stored=False):
        """:meth:`RawKNNRegressor._bootstrap_request` of a streamed call, kept as ``request``: every other product and the
        call's neighbour keywords do not go with a bootstrap and are refused when set."""
        self.request = est._bootstrap_request(
            self.bootstrap, statistic, outputs, n_targets=n_targets, stored=stored, zonal=self.zonal, zones=self.zones,
            usage=self.usage, domain=self.domain, domain_out=self.domain_out,
            beyond=None if self.beyond == "keep" else self.beyond, return_neighbors=bool(return_neighbors) or None,
            return_dataframe_index=bool(return_dataframe_index) or None, neighbors_out=neighbors_out,
            index_dtype=index_dtype, distance_dtype=distance_dtype)
        return self.request

    # -- open ----------------------------------------------------------------------------------------
    def open_keywords(self, eng, n_neighbors) -> dict:
        """The product keywords of ``eng.open_stream`` / ``eng.open_replay`` (their tuples: ``Index.open_stream``); a
        bootstrap's table is handed to the engine on the way, and its replicates hold ``n_neighbors`` copies."""
        kw = {}
        if self.usage is not None:
            kw["tally"] = True
        if self.zonal is not None:
            kw["zonal"] = (self.zonal.n_zones, self.zonal.n_classes(self._zonal_binding[0]))
        if self.domain is not None:
            kw["domain"] = (self.domain.table, self.domain.rank, self.domain.threshold, self.blank)
        if self.bootstrap is not None:
            eng.set_bootstrap(self.request[2])
            kw["bootstrap"] = (n_neighbors, self.request[1])
        return kw

    # -- feed ----------------------------------------------------------------------------------------
    def next_tile(self):
        """For EVERY tile, before it is looked at: in lockstep, a skipped empty tile consumes its zone codes too."""
        if self.zonal is not None:
            try:
                self._tile_zones = next(self.zones)
            except StopIteration:
                raise ValueError(_ZONES_SHORT) from None

    def feed(self, stream, row, n):
        """Before the push of a tile of ``n`` pixels, the call's pixels ``[row, row + n)``."""
        if self.zonal is not None:
            stream.next_zones(normalize_zone_tile(self._tile_zones, n))
        if self.domain_out is not None:
            if self.domain_out.size < row + n:
                raise ValueError(f"domain_out holds {self.domain_out.size} pixels: the tiles hold at least {row + n}")
            stream.next_domain_out(self.domain_out[row:row + n])

    def end_of_tiles(self):
        if self.zonal is not None and next(self.zones, None) is not None:
            raise ValueError(_ZONES_LONG)

    # -- collect and commit --------------------------------------------------------------------------
    def collect(self, stream):
        """Read the stream's accumulators; the caller closes the stream afterwards, whatever this raises."""
        wanted = dict(tally=self.usage, zonal=self.zonal, domain=self.domain, bootstrap=self.bootstrap)
        self._collected = {name: getattr(stream, name)() for name, product in wanted.items() if product is not None}

    def commit(self, est, k):
        """Add what :meth:`collect` read to the user's objects -- only a call that came through whole is added.  Without
        a stream (no tile held a pixel) ``zonal`` and ``usage`` are bound all the same, ``usage`` to ``k`` neighbours."""
        got = self._collected
        if "bootstrap" in got:
            self.bootstrap._add(got["bootstrap"])
        if "domain" in got:
            self.domain._add(got["domain"])
        if self.zonal is not None:
            self.zonal._bind(*self._zonal_binding)
            if "zonal" in got:
                self.zonal._add(*got["zonal"])
        if self.usage is not None:
            ids = getattr(est, "dataframe_index_in_", None)
            if "tally" in got:
                self.usage._add(*got["tally"], ids)
            else:
                self.usage._bind(est.n_samples_fit_, k, ids)
