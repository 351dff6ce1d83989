"""Float64 interval reference of the standard Hough transform, cv::HoughLines(image, lines, rho, theta,
threshold), written from its definition.  TEST INFRASTRUCTURE ONLY.  It shares nothing with
RoadEstimation::HoughLines or k_road_hough but the definition itself:

  * the angles  ang_0 = 0, ang_{n+1} = fp32(ang_n + theta),  numangle = round(pi / theta);
  * numrho = round(((W + H) * 2 + 1) / rho)  for an image of H rows and W columns;
  * an accumulator of (numangle + 2) x (numrho + 2) cells with a border of zeros; the pixel (row i, column j)
    votes, for every angle n, for the cell r = round(j * cos(ang_n) / rho + i * sin(ang_n) / rho) + (numrho - 1) / 2;
  * a cell is a line when its votes v satisfy  v > threshold, v > left, v >= right, v > up, v >= down
    (left / right: r -+ 1, up / down: n -+ 1);
  * lines ordered by votes descending, then by accumulator index (n + 1) * (numrho + 2) + r + 1 ascending;
  * the output (rho, theta) = ((r - (numrho - 1) * 0.5) * rho, n * theta) in fp32.

The vote and its interval.  An implementation evaluates the vote in fp32: table entries fp32(cos(ang_n)),
fp32(sin(ang_n)), the two products rounded to fp32, their sum rounded to fp32, then round-to-nearest.  This
module evaluates v64 = j * cos(ang_n) + i * sin(ang_n) in float64 and bounds how far the fp32 value can lie from
it, for rho = 1 (the only resolution in use; any other raises).  With u = 2^-24 (half an fp32 ulp, relative) and
0 <= j < W, 0 <= i < H:

  * a table entry is off by at most u * |cos| <= u from the float64 value, so j * tab is off by at most j * u;
  * each product is rounded once more: at most u * j resp. u * i on top;
  * the sum of the two rounded products has magnitude at most W + H and is rounded once: at most u * (W + H);
  * float64's own error, (W + H) * 2^-52 or so, vanishes beside these.

Together: |v32 - v64| <= (j + i) * 2u + (W + H) * u <= 3 * (W + H) * 2^-24 < (W + H) * 2^-22 = DELTA.  The bound
is derived, not measured, and is generous by a third on purpose.  A vote whose v64 lies farther than DELTA from
every half-integer rounds to the same cell in both precisions: it is CERTAIN.  Otherwise it is AMBIGUOUS and
may land in either of the two cells beside that half-integer.  Per cell:

  lo  = the certain votes,
  hi  = lo + every ambiguous vote that could land there (such a vote counts towards hi of both its cells),
  nominal = the votes with v64 itself rounded (half to even), lo <= nominal <= hi; where nothing is ambiguous the
            three are equal and `lines()` is THE answer, bit for bit.

From lo / hi follow the cells that are peaks whatever the ambiguous votes do (`certain_peaks`: lo of the cell
against hi of its neighbours) and the cells that can be peaks at all (`possible_peaks`: hi against lo).
"""
import numpy as np

THETA = np.float32(np.float32(3.14159274) / np.float32(180.0))   # fp32(CV_PI / 180), the angle step in use


class Hough:
    """Bounds of the accumulator of one image.  lo, hi, nominal: int64 [numangle + 2][numrho + 2], zero border."""

    def __init__(self, image, rho=1.0, theta=THETA, threshold=25, chunk=4096):
        image = np.asarray(image)
        if image.ndim != 2:
            raise ValueError("a 2-D image is expected")
        if float(rho) != 1.0:
            raise NotImplementedError("DELTA is derived for rho = 1 only")
        H, W = image.shape
        self.rho, self.theta, self.threshold = np.float32(rho), np.float32(theta), int(threshold)
        self.numangle = int(np.rint(np.pi / np.float64(self.theta)))
        self.numrho = int(np.rint(((W + H) * 2 + 1) / np.float64(self.rho)))
        self.delta = (W + H) * 2.0 ** -22
        ang = np.zeros(self.numangle, np.float32)
        for n in range(1, self.numangle):                     # the definition's fp32 running sum
            ang[n] = np.float32(ang[n - 1] + self.theta)
        c64, s64 = np.cos(ang.astype(np.float64)), np.sin(ang.astype(np.float64))
        stride, half = self.numrho + 2, (self.numrho - 1) // 2
        cells = (self.numangle + 2) * stride
        row0 = (np.arange(self.numangle, dtype=np.int64) + 1) * stride + half + 1    # cell of r = 0 per angle
        lo, amb, nominal = (np.zeros(cells, np.int64) for _ in range(3))
        ii, jj = np.nonzero(image)
        self.n_points, self.n_votes, self.n_ambiguous = len(ii), len(ii) * self.numangle, 0
        for a in range(0, len(ii), chunk):
            v = (np.multiply.outer(jj[a:a + chunk].astype(np.float64), c64)
                 + np.multiply.outer(ii[a:a + chunk].astype(np.float64), s64))       # [points][angles]
            below = np.floor(v)
            unsure = np.abs(v - below - 0.5) <= self.delta
            cell = row0[None, :] + below.astype(np.int64)       # the cell below the nearest half-integer
            up = (v - below > 0.5).astype(np.int64)
            lo += np.bincount((cell + up)[~unsure], minlength=cells)
            amb += np.bincount(cell[unsure], minlength=cells) + np.bincount(cell[unsure] + 1, minlength=cells)
            nominal += np.bincount((row0[None, :] + np.rint(v).astype(np.int64)).ravel(), minlength=cells)
            self.n_ambiguous += int(unsure.sum())
        shape = (self.numangle + 2, stride)
        self.lo, self.hi, self.nominal = lo.reshape(shape), (lo + amb).reshape(shape), nominal.reshape(shape)
        for acc in (self.lo, self.hi, self.nominal):            # every vote stays inside the border
            assert not acc[0].any() and not acc[-1].any() and not acc[:, 0].any() and not acc[:, -1].any()

    def _peaks(self, own, other):
        """Interior cells [numangle][numrho] whose `own` count wins against the `other` counts of the four
        neighbours by the rule of the definition."""
        c = own[1:-1, 1:-1]
        return ((c > self.threshold) & (c > other[1:-1, :-2]) & (c >= other[1:-1, 2:])
                & (c > other[:-2, 1:-1]) & (c >= other[2:, 1:-1]))

    def certain_peaks(self):
        return self._peaks(self.lo, self.hi)

    def possible_peaks(self):
        return self._peaks(self.hi, self.lo)

    def line(self, n, r):
        """The fp32 (rho, theta) the definition reports for the cells (n, r)."""
        n, r = np.asarray(n), np.asarray(r)
        out = np.empty(n.shape + (2,), np.float32)
        out[..., 0] = (r.astype(np.float32) - np.float32((self.numrho - 1) * 0.5)) * self.rho
        out[..., 1] = n.astype(np.float32) * self.theta
        return out

    def lines(self):
        """(lines [K][2] fp32, n [K], r [K], votes [K]) of the nominal accumulator, in the definition's order."""
        n, r = np.nonzero(self._peaks(self.nominal, self.nominal))
        votes = self.nominal[n + 1, r + 1]
        order = np.lexsort(((n + 1) * (self.numrho + 2) + r + 1, -votes))
        n, r, votes = n[order], r[order], votes[order]
        return self.line(n, r), n, r, votes

    def decode(self, lines):
        """The cells (n [K], r [K]) of reported lines; raises if one is not the fp32 image of a cell."""
        lines = np.asarray(lines, np.float32).reshape(-1, 2)
        n = np.rint(lines[:, 1].astype(np.float64) / np.float64(self.theta)).astype(np.int64)
        r = np.rint(lines[:, 0].astype(np.float64) / np.float64(self.rho) + (self.numrho - 1) * 0.5).astype(np.int64)
        if ((n < 0) | (n >= self.numangle) | (r < 0) | (r >= self.numrho)).any():
            raise ValueError("a line lies outside the accumulator")
        if not np.array_equal(self.line(n, r).view(np.int32), lines.view(np.int32)):
            raise ValueError("a line is not the fp32 image of an accumulator cell")
        return n, r

    def index(self, n, r):
        return (np.asarray(n) + 1) * (self.numrho + 2) + np.asarray(r) + 1

    def dominant(self, n, r, among=None):
        """True if (n, r) is a certain peak whose lo exceeds hi of every other possible peak: it heads the list of
        every implementation inside the bounds.  `among` (bool [numangle][numrho]) narrows the rivals, e.g. to the
        cells whose line passes a gate: then (n, r) heads every such list after the gate."""
        others = self.possible_peaks()
        if among is not None:
            others &= among
        if not self.certain_peaks()[n, r]:
            return False
        others[n, r] = False
        rivals = self.hi[1:-1, 1:-1][others]
        return bool(rivals.size == 0 or self.lo[n + 1, r + 1] > rivals.max())

    def determined(self):
        """True if the bounds leave one list only: every possible peak is certain and no ambiguous vote touches a
        peak.  Then `lines()` is exact although the image has ambiguous votes elsewhere."""
        certain, possible = self.certain_peaks(), self.possible_peaks()
        return bool(np.array_equal(certain, possible)
                    and np.array_equal(self.lo[1:-1, 1:-1][certain], self.hi[1:-1, 1:-1][certain]))

    def check_lines(self, lines, votes=None, complete=True):
        """Asserts that a reported list lies inside the bounds: every line is a possible peak, reported once; every
        certain peak is reported (`complete`: the list was not cut short); the order is one that some assignment of
        the ambiguous votes gives.  With the implementation's `votes`: lo <= votes <= hi, non-increasing, equal votes
        by ascending accumulator index."""
        n, r = self.decode(lines)
        idx = self.index(n, r)
        assert len(np.unique(idx)) == len(idx), "a cell is reported twice"
        possible = self.possible_peaks()
        bad = np.nonzero(~possible[n, r])[0]
        assert bad.size == 0, f"line {bad[0]} = cell (n {n[bad[0]]}, r {r[bad[0]]}) cannot be a peak"
        if complete:
            missing = self.certain_peaks()
            missing[n, r] = False
            assert not missing.any(), f"certain peaks not reported: {np.argwhere(missing)[:5].tolist()}"
        lo, hi = self.lo[n + 1, r + 1], self.hi[n + 1, r + 1]
        if votes is None:
            # some assignment must put line k at or above every later line ...
            later = np.maximum.accumulate(lo[::-1])[::-1]
            assert (hi[:-1] >= later[1:]).all(), "the order contradicts the bounds"
            # ... and where two neighbours' votes are known and equal, the index decides
            known = (lo[:-1] == hi[:-1]) & (lo[1:] == hi[1:]) & (lo[:-1] == lo[1:])
            assert (idx[1:][known] > idx[:-1][known]).all(), "equal votes out of index order"
        else:
            votes = np.asarray(votes, np.int64)
            assert len(votes) == len(idx)
            assert ((lo <= votes) & (votes <= hi)).all(), "votes outside [lo, hi]"
            assert (votes > self.threshold).all()
            assert (np.diff(votes) <= 0).all(), "votes increase along the list"
            tie = np.diff(votes) == 0
            assert (idx[1:][tie] > idx[:-1][tie]).all(), "equal votes out of index order"
