"""The folder rules of the mesh commands (__main__.py), free of the device: which files a command reads, where it writes,
what it skips and what it returns.  A command supplies callables that do the work of one file; the walks here own the rest.

Listing.  ``obj_files`` is the sorted listing of FOLDER/*.obj with the folder's name taken literally; ``noisy_of`` the
NAME_n*.obj of one original (the stem taken literally too: ``a[x]`` is a name, no character class).  ``box_n*.obj`` also
matches ``box_new_n1.obj``: a stem that continues another with ``_n`` is paired with both -- known, and left as it is.
``originals`` lists DIR/original if that folder exists, else DIR itself (`clean`, `subdivide`, `decimate`, `fill`, `remesh`,
`info`, `sample`); `noise` lists DIR/original only.

Order.  Files in sorted order; in the paired walk every original is followed by its noisy files in sorted order.  One
printed line per written file, flushed.

Output folders.  The paired walk writes OUT/original and OUT/noisy when DIR/original exists -- OUT/noisy is made even when
DIR/noisy is absent -- and OUT alone otherwise.  `remesh` carries no noisy files along and makes no OUT/noisy; `remesh
--project` with DIR/original and DIR/noisy present is a paired walk like the others.  `project` pairs as `align` does and
writes OUT alone.

Skips.  ``walk`` catches ValueError, OSError and GeobiError around the work of one file, prints ``skipped: ...`` on stderr
and counts one file, however much of it was done (`noise`: a failure part-way through the levels is one file).  In the
paired walk a noisy file of another size than its original is refused with one message, counted, and the walk goes on to
the next noisy file; this inner handler catches ValueError and OSError only, so a GeobiError from ``apply`` ends that
stem through the outer handler and counts once (what the inner handler counted before stays counted).

Trailer.  ``\\n--- end ---`` on stdout, then on stderr, if anything was skipped, ``N files skipped`` (of_total=False:
`clean`, `subdivide`, `decimate`, `fill`, `remesh`) or ``N of M files skipped`` (`info`, `sample`, `noise`, `align`,
`project`).  The return value is 1 if anything was skipped or there was no file at all, else 0.
"""
import glob
import os
import sys

from . import meshio
from ._lib import GeobiError


def obj_files(folder, pattern='*'):
    """sorted FOLDER/<pattern>.obj; the folder's name is escaped, the pattern is a glob pattern"""
    return sorted(glob.glob(os.path.join(glob.escape(folder), pattern + '.obj')))


def variants_of(folder, stem, tail='_*'):
    """sorted FOLDER/STEM<tail>.obj, the stem taken literally: the results or the sources that belong to STEM.obj"""
    return obj_files(folder, glob.escape(stem) + tail)


def noisy_of(noisy_dir, stem):
    """sorted NOISY_DIR/STEM_n*.obj: the noisy files of original/STEM.obj"""
    return variants_of(noisy_dir, stem, '_n*')


def stem_of(path):
    """NAME of a path that ends in NAME.obj"""
    return os.path.basename(path)[:-4]


def originals(data_dir):
    """-> (the files of DIR/original if that folder exists, else of DIR; whether it exists)"""
    original_dir = os.path.join(data_dir, 'original')
    paired = os.path.isdir(original_dir)
    return obj_files(original_dir if paired else data_dir), paired


def walk(jobs, one, of_total=True):
    """``one(job, skip)`` for every job in order; it does the work of one file and prints that file's lines.  What it raises
    (ValueError, OSError, GeobiError) skips the rest of the job and counts one file; ``skip(error)`` reports and counts a
    file the callable gives up on its own and goes on.  Prints the end line and the trailer; -> the command's return value."""
    failed = 0

    def skip(error):
        nonlocal failed
        failed += 1
        print('skipped: %s' % error, file=sys.stderr, flush=True)

    for job in jobs:
        try:
            one(job, skip)
        except (ValueError, OSError, GeobiError) as e:
            skip(e)
    print('\n--- end ---')
    if failed:
        print('%d of %d files skipped' % (failed, len(jobs)) if of_total else '%d files skipped' % failed, file=sys.stderr)
    return 1 if failed or not jobs else 0


def paired_walk(data_dir, out_dir, title, plan, mesh_of, line, apply):
    """A tool over a folder and its paired noisy files.  ``plan(points, faces, path) -> result`` works on one original as
    read (the path is for its messages), ``mesh_of(result) -> (points, faces)`` as numpy is what gets written,
    ``apply(result, noisy_points) -> points`` as numpy replays the plan on a paired array, ``line(result, V, F, out_file)``
    is the printed line of every written file (V, F: the original's sizes).  Prints ``\\nTITLE, M files ...\\n`` first."""
    files, paired = originals(data_dir)
    out_original = os.path.join(out_dir, 'original') if paired else out_dir
    os.makedirs(out_original, exist_ok=True)
    if paired:
        os.makedirs(os.path.join(out_dir, 'noisy'), exist_ok=True)
    print('\n%s, %d files ...\n' % (title, len(files)), flush=True)

    def one(path, skip):
        points, faces = meshio.read_obj(path)
        V, F = points.shape[0], faces.shape[0]
        result = plan(points, faces, path)
        points_out, faces_out = mesh_of(result)
        out_file = os.path.join(out_original, os.path.basename(path))
        meshio.write_obj(out_file, points_out, faces_out)
        print(line(result, V, F, out_file), flush=True)
        if not paired:
            return
        for noisy in noisy_of(os.path.join(data_dir, 'noisy'), stem_of(path)):
            try:
                n_points, n_faces = meshio.read_obj(noisy)
                if n_points.shape != points.shape or n_faces.shape != faces.shape:
                    raise ValueError('%s (V = %d, F = %d) and its original %s (V = %d, F = %d) differ in size'
                                     % (noisy, n_points.shape[0], n_faces.shape[0], path, V, F))
                out_file = os.path.join(out_dir, 'noisy', os.path.basename(noisy))
                meshio.write_obj(out_file, apply(result, n_points), faces_out)
                print(line(result, V, F, out_file), flush=True)
            except (ValueError, OSError) as e:
                skip(e)

    return walk(files, one, of_total=False)
